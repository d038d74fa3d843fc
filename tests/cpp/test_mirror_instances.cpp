// tests/test_instances.py (g++ against libyhair.so, no GPU): an instanced scene file through yh_scene_load and the C++ mirror's
// init_scene (host/yscene_cli.h), as both command lines convert it: one ptr::object per frame of the instance file, each
// with the composed frame and its object's shape and material. argv[1]: the scene, argv[2]: the number of objects expected.
#include "yscene_cli.h"

int main(int argc, const char* argv[]) {
  if (argc < 3) return 2;
  char err[512] = "";
  auto file = yh_scene_load(argv[1], "", err, sizeof(err));
  if (!file) {
    printf("%s\n", err);
    return 3;
  }
  auto       d = yh_scene_get(file);
  ptr::scene scene;
  init_scene(&scene, d, yh_scene_get_maps(file));
  if (d->num_objects != atoi(argv[2]) || (int)scene.objects.size() != d->num_objects) return 4;
  for (int i = 0; i < d->num_objects; i++) {
    if (memcmp(&scene.objects[(size_t)i]->frame, d->objects[i].frame, 48)) return 5;
    if (scene.objects[(size_t)i]->shape_ != scene.shapes[(size_t)d->objects[i].shape].get()) return 6;
    if (scene.objects[(size_t)i]->material_ != scene.materials[(size_t)d->objects[i].material].get()) return 7;
  }
  printf("%d objects, %d shapes\n", (int)scene.objects.size(), (int)scene.shapes.size());
  yh_scene_free(file);
  return 0;
}
