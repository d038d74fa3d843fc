// Compile check (tests/test_material_maps.py, g++ only, no GPU): a scene built through the C++ mirror of the reference's
// scene API with the texture arguments of its material setters (yocto_pathtrace.h:134-148) — scalar maps on specular,
// metallic, roughness, transmission and opacity, a normal map through set_normalmap, scalar images in 8-bit and float
// through the set_texture overloads of yocto_pathtrace.h:117-118 — as a caller of the reference writes it.
#include "yhair_pathtrace.h"

namespace ptr = yhair::pathtrace;
using yhair::math::vec3f;

ptr::material* mapped_material(ptr::scene* scene) {
  auto grey_bytes = ptr::add_texture(scene);
  ptr::set_texture(grey_bytes, 2, 2, std::vector<unsigned char>{0, 64, 128, 255});
  auto grey_floats = ptr::add_texture(scene);
  ptr::set_texture(grey_floats, 2, 1, std::vector<float>{0.25f, 0.75f});
  auto normals = ptr::add_texture(scene);
  ptr::set_texture(normals, 1, 1, std::vector<ptr::vec3b>{{128, 128, 255}});
  auto material = ptr::add_material(scene);
  ptr::set_color(material, vec3f{0.5f, 0.5f, 0.5f}, nullptr);
  ptr::set_specular(material, 1, grey_bytes);
  ptr::set_metallic(material, 0.5f, grey_floats);
  ptr::set_roughness(material, 0.3f, grey_bytes);
  ptr::set_transmission(material, 0, false, 0.01f, grey_floats);
  ptr::set_opacity(material, 0.9f, grey_bytes);
  ptr::set_normalmap(material, normals);
  ptr::set_specular(material);  // the defaults of the reference's signatures still apply
  ptr::set_specular(material, 1, grey_bytes);
  return material;
}

int main() {
  ptr::scene scene;
  return mapped_material(&scene)->normal_tex && scene.textures[0]->colorb.size() == 4 &&
                 scene.textures[1]->colorf[1].y == 0.75f
             ? 0
             : 1;
}
