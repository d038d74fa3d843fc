// The planes of yh_gbuffer by name (yocto-hair_amd/host/image_planes.h), without a device: their order and bytes per pixel against the
// struct of include/yhair.h, which planes the a-trous filter, the temporal step and yh_temporal_display read, and the name of the first
// plane a caller left out. Every expectation below is written out by hand from include/yhair.h (GBUFFER: the table of planes; DENOISE:
// "the planes the parameters read"; TEMPORAL), none is computed by the header under test.
#include <cstdio>
#include <cstring>

#include "image_planes.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) printf("FAILED line %d: %s\n", __LINE__, #cond), failures++; \
  } while (0)

// the bits, by hand: the position of each plane in yh_gbuffer
enum : unsigned { OBJECT = 1u << 0, POSITION = 1u << 5, NORMAL = 1u << 6, ALBEDO = 1u << 9 };

static yh_denoise_params params(int iterations, float sigma_normal, float sigma_position, int demodulate) {
  yh_denoise_params p;
  memset(&p, 0, sizeof(p));
  p.iterations = iterations, p.sigma_color = 4.0f, p.sigma_normal = sigma_normal, p.sigma_position = sigma_position, p.demodulate = demodulate;
  return p;
}
static bool same(const char* a, const char* b) { return a && b && strcmp(a, b) == 0; }

int main() {
  // ---- order and sizes, against the struct ----
  CHECK(PLANES == 11 && sizeof(yh_gbuffer) == 11 * sizeof(void*));
  {
    int   i[3];
    float f[8];
    yh_gbuffer g;
    g.object = i, g.element = i + 1, g.material = i + 2, g.uv = f, g.distance = f + 1, g.position = f + 2, g.normal = f + 3, g.tangent = f + 4, g.texcoord = f + 5,
    g.albedo = f + 6, g.ray = f + 7;
    const void*  member[11] = {g.object, g.element, g.material, g.uv, g.distance, g.position, g.normal, g.tangent, g.texcoord, g.albedo, g.ray};
    const char*  name[11]   = {"object", "element", "material", "uv", "distance", "position", "normal", "tangent", "texcoord", "albedo", "ray"};
    const size_t bytes[11]  = {4, 4, 4, 8, 4, 12, 12, 12, 8, 12, 24};  // int, int, int, float2, float, float3, float3, float3, float2, float3, 6 float
    for (int k = 0; k < 11; k++) {
      CHECK(plane_of(g, k) == member[k]);
      CHECK(same(plane_name[k], name[k]));
      CHECK(plane_bytes[k] == bytes[k]);
    }
    CHECK(PLANE_object == 0 && PLANE_element == 1 && PLANE_material == 2 && PLANE_uv == 3 && PLANE_distance == 4 && PLANE_position == 5);
    CHECK(PLANE_normal == 6 && PLANE_tangent == 7 && PLANE_texcoord == 8 && PLANE_albedo == 9 && PLANE_ray == 10);
    CHECK(planes_present(g) == 0x7ffu);
    // set_plane writes the member it names and no other
    yh_gbuffer h;
    memset(&h, 0, sizeof(h));
    set_plane(h, PLANE_normal, f);
    CHECK(h.normal == f && planes_present(h) == NORMAL);
    set_plane(h, PLANE_ray, f + 1);
    CHECK(h.ray == f + 1 && h.normal == f && planes_present(h) == (NORMAL | 1u << 10));
    // planes_in keeps the planes of the mask and drops the rest
    const yh_gbuffer r = planes_in(OBJECT | ALBEDO, g);
    CHECK(r.object == i && r.albedo == f + 6 && planes_present(r) == (OBJECT | ALBEDO));
    CHECK(planes_present(planes_in(0, g)) == 0);
  }

  // ---- the filter's mask: object always; normal iff sigma_normal > 0; position iff sigma_position > 0; albedo iff demodulate ----
  {
    yh_denoise_params p;
    p = params(5, 0.0f, 0.0f, 0); CHECK(filter_planes(&p) == OBJECT);
    p = params(5, 0.5f, 0.0f, 0); CHECK(filter_planes(&p) == (OBJECT | NORMAL));
    p = params(5, 0.0f, 2.0f, 0); CHECK(filter_planes(&p) == (OBJECT | POSITION));
    p = params(5, 0.5f, 2.0f, 0); CHECK(filter_planes(&p) == (OBJECT | NORMAL | POSITION));
    p = params(5, 0.0f, 0.0f, 1); CHECK(filter_planes(&p) == (OBJECT | ALBEDO));
    p = params(5, 0.5f, 0.0f, 1); CHECK(filter_planes(&p) == (OBJECT | NORMAL | ALBEDO));
    p = params(5, 0.0f, 2.0f, 1); CHECK(filter_planes(&p) == (OBJECT | POSITION | ALBEDO));
    p = params(5, 0.5f, 2.0f, 1); CHECK(filter_planes(&p) == (OBJECT | NORMAL | POSITION | ALBEDO));
    p = params(1, 0.5f, 2.0f, 1); CHECK(filter_planes(&p) == (OBJECT | NORMAL | POSITION | ALBEDO));  // (one level reads what five read)
    p = params(5, -1.0f, -1.0f, 0); CHECK(filter_planes(&p) == OBJECT);  // (a negative sigma switches its term off, as zero does)
    // no level, or no parameters: the filter does not run and reads nothing
    p = params(0, 0.5f, 2.0f, 1); CHECK(filter_planes(&p) == 0);
    CHECK(filter_planes(nullptr) == 0);
  }

  // ---- the temporal step, and the one pass yh_temporal_display traces for both stages ----
  {
    CHECK(temporal_planes() == (OBJECT | POSITION));
    yh_denoise_params p;
    CHECK(display_planes(nullptr) == (OBJECT | POSITION));
    p = params(0, 0.5f, 2.0f, 1); CHECK(display_planes(&p) == (OBJECT | POSITION));
    p = params(5, 0.0f, 0.0f, 0); CHECK(display_planes(&p) == (OBJECT | POSITION));  // (position: the temporal step's)
    p = params(5, 0.5f, 0.0f, 0); CHECK(display_planes(&p) == (OBJECT | POSITION | NORMAL));
    p = params(5, 0.0f, 2.0f, 1); CHECK(display_planes(&p) == (OBJECT | POSITION | ALBEDO));
    p = params(5, 0.5f, 2.0f, 1); CHECK(display_planes(&p) == (OBJECT | POSITION | NORMAL | ALBEDO));
  }

  // ---- the first missing plane, by name ----
  {
    int   i[1];
    float f[3];
    const unsigned all = OBJECT | NORMAL | POSITION | ALBEDO;
    yh_gbuffer     g;
    memset(&g, 0, sizeof(g));
    g.object = i, g.normal = f, g.position = f + 1, g.albedo = f + 2;
    CHECK(missing_plane(all, g) == nullptr);
    CHECK(missing_plane(0, g) == nullptr);
    yh_gbuffer m;
    m = g, m.object = nullptr; CHECK(same(missing_plane(all, m), "object"));
    m = g, m.normal = nullptr; CHECK(same(missing_plane(all, m), "normal"));
    m = g, m.position = nullptr; CHECK(same(missing_plane(all, m), "position"));
    m = g, m.albedo = nullptr; CHECK(same(missing_plane(all, m), "albedo"));
    // a plane outside the mask is not missed
    m = g, m.normal = nullptr; CHECK(missing_plane(OBJECT | POSITION | ALBEDO, m) == nullptr);
    m = g, m.albedo = nullptr; CHECK(missing_plane(temporal_planes(), m) == nullptr);
    // with several missing, the order the refusals have always named them in: object, normal, position, albedo
    memset(&m, 0, sizeof(m));
    CHECK(same(missing_plane(all, m), "object"));
    m.object = i; CHECK(same(missing_plane(all, m), "normal"));
    m.normal = f; CHECK(same(missing_plane(all, m), "position"));
    m.position = f; CHECK(same(missing_plane(all, m), "albedo"));
    memset(&m, 0, sizeof(m));
    CHECK(same(missing_plane(temporal_planes(), m), "object"));
    m.object = i; CHECK(same(missing_plane(temporal_planes(), m), "position"));
    // the unit-level entries' four loose pointers as a yh_gbuffer
    const yh_gbuffer u = guides_of(i, f, f + 1, f + 2);
    CHECK(u.object == i && u.normal == f && u.position == f + 1 && u.albedo == f + 2 && planes_present(u) == all);
  }

  if (failures) return printf("%d checks FAILED\n", failures), 1;
  printf("all checks passed\n");
  return 0;
}
