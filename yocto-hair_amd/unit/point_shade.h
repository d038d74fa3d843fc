// point_shade.h — the body of the unit-level shading-point kernels (yh_point_batch): what the sample loops make of a closest hit before
// the lobes are sampled — the head of path_step / shade_step (dev_path.h) up to surface_brdf — row by row on the uploaded scene with its
// maps. Every step calls the device functions of dev_path.h / dev_surface.h themselves, in the order the head of path_step calls them:
//     the object and material rows          from LDS (stage_tables) or from memory, as the loop the form stands for reads them
//     eval_hit_fetch_first / eval_hit       position, eval_normal
//     eval_hit_maps                         texcoord, eval_normalmap, eval_maps (the variants that know maps)
//     the shading-normal rule               quad_orthonormalize for a strand, the thin flip for a triangle
//     eval_texcoord, eval_texture           colour, emission (and its linear .x) and, for the column alone, scattering
//     surface_brdf                          the mixture — or, where the loop computes none (a plain material on a plain variant), what
//                                           its diffuse-only path uses: the colour, opacity 1, the row's diffuse_pdf
//     medium_crossing                       from outside, incoming = -outgoing
//
// Compiled twice, as the sample loop is: unit/point_quad.hip (a quad per row: forms 0 and 2) and unit/point_lane.hip with YH_LANE 1 (a
// lane per row: form 1). FORM x GENERAL (the scene's variant, as a launch settles it) select the code as the loops' template arguments do:
//     form 0, plain scene     path_step<.., GENERAL = false, TRIM = true>: rows from LDS, eval_hit_fetch_first, no maps, no mixture
//     form 0, general scene   path_step<.., GENERAL = true>: rows from memory, eval_hit + eval_hit_maps, the mixture unless the row is plain
//     form 1                  k_stream's path_step<false, 64, GENERAL> under YH_LANE: rows from LDS on a plain scene, else as form 0's
//     form 2                  shade_step, and the rows of the 256-thread path_step: rows from memory whatever the scene, eval_hit +
//                             eval_hit_maps for every material, the mixture always (with path_step's rule for when the texcoord is
//                             needed, which adds the scattering texture: shade_step knows no medium)
// out, YH_POINT_FLOATS per row: the columns of include/yhair.h (YH_POINT_*).
#include <hip/hip_runtime.h>

#include "yhair.h"
#include "dev_path.h"

using namespace yhd;

template <int FORM, bool GENERAL>
YH_DEV void point_row(const trace_ctx& tc, const hit_t& isec, f3 outgoing, yhd_float4* slot, bool write, float* out) {
  const yhd_scene& sc    = *tc.sc;
  constexpr bool   SHADE = FORM == 2;
  constexpr bool   TRIM  = FORM == 0 && !GENERAL;
  constexpr bool   MAPS  = GENERAL || SHADE;  // eval_hit_maps and the mixture are compiled in
  constexpr bool   from_lds = !SHADE && !GENERAL;
  const yhd_object&   o   = !from_lds ? sc.objects[isec.object] : *(const yhd_object*)(const YH_LDS yhd_object*)(tc.lds_scene + YH_OBJECT_F4 * isec.object);
  const yhd_material& mat = !from_lds ? sc.materials[o.material] : *(const yhd_material*)(const YH_LDS yhd_material*)(tc.lds_mats + YH_MATERIAL_F4 * o.material);
  hit_geom hg;
  if constexpr (TRIM) hg = eval_hit_fetch_first(sc, o, isec.slot, isec.u, isec.v);
  else hg = eval_hit(sc, o, isec.slot, isec.u, isec.v);
  f3 position = hg.position;
  f3 nrm      = hg.normal;
  hit_maps hm;
  if constexpr (MAPS) hm = eval_hit_maps(sc, o, isec, SHADE || !mat.plain, nrm);
  f3   normal;  // eval_shading_normal (pt.cpp:350-369)
  bool is_hair = o.kind == YH_KIND_LINES;
  if (is_hair) {
    normal = quad_orthonormalize(outgoing, nrm);
  } else {
    normal = (!mat.thin || dot(nrm, outgoing) >= 0) ? nrm : -nrm;
  }
  const bool     general = SHADE || (GENERAL && !mat.plain);
  surface_brdf_t sb;
  float          tu = isec.u, tv = isec.v, etex_x = 1.0f;
  f3             ctex = mk3(1.0f), etex = mk3(1.0f), stex = mk3(1.0f);
  if (general) {
    if constexpr (MAPS) tu = hm.tu, tv = hm.tv;
    if (mat.color_tex >= 0 || mat.emission_tex >= 0 || mat.scattering_tex >= 0) {
      if constexpr (MAPS) {
        if (!hm.have_tc) eval_texcoord(sc, o, isec, tu, tv);
      }
      ctex = eval_texture(sc, mat.color_tex, false, tu, tv);
      if (mat.emission_tex >= 0) {
        etex   = eval_texture(sc, mat.emission_tex, false, tu, tv);
        etex_x = eval_texture(sc, mat.emission_tex, true, tu, tv).x;
      }
      stex = eval_texture(sc, mat.scattering_tex, false, tu, tv);  // (the loop looks it up inside medium_crossing)
    }
    if constexpr (MAPS) sb = surface_brdf(mat, normal, outgoing, ctex, etex_x, hm.f);
    else sb = surface_brdf(mat, normal, outgoing, ctex, etex_x);
  } else {  // the diffuse-only path of path_step: no mixture is made, these are the values it works with
    sb.diffuse = ld3(mat.color), sb.specular = sb.metal = sb.transmission = sb.refraction = mk3(0.0f);
    sb.roughness = 1.0f, sb.opacity = 1.0f;
    sb.diffuse_pdf = mat.diffuse_pdf, sb.specular_pdf = sb.metal_pdf = sb.transmission_pdf = sb.refraction_pdf = 0.0f;
  }
  const f3 emission = ld3(mat.emission) * etex;
  path_t   ps;
  ps.in_medium      = false;
  ps.medium.density = mk3(0.0f), ps.medium.scatter = mk3(0.0f), ps.medium.anisotropy = 0.0f;
#if YH_LANE
  ps.medium_mem = slot;
#endif
  if (general) medium_crossing(sc, ps, mat, normal, outgoing, -outgoing, ctex, etex_x, tu, tv);
#if YH_LANE
  if (ps.in_medium) {  // (as path_step: the medium comes back from the path's slot)
    const yhd_float4 m0 = ps.medium_mem[0], m1 = ps.medium_mem[1];
    ps.medium.density = f3{m0.x, m0.y, m0.z}, ps.medium.anisotropy = m0.w, ps.medium.scatter = f3{m1.x, m1.y, m1.z};
  }
#endif
  if (!write) return;
  auto put3 = [&](int at, f3 a) { out[at] = a.x, out[at + 1] = a.y, out[at + 2] = a.z; };
  put3(YH_POINT_POSITION, position), put3(YH_POINT_NORMAL, hg.normal), put3(YH_POINT_SHADING_NORMAL, normal);
  out[YH_POINT_TEXCOORD] = tu, out[YH_POINT_TEXCOORD + 1] = tv;
  put3(YH_POINT_COLOR_TEX, ctex), put3(YH_POINT_EMISSION_TEX, etex), out[YH_POINT_EMISSION_TEX_X] = etex_x;
  put3(YH_POINT_SCATTERING_TEX, stex), put3(YH_POINT_EMISSION, emission);
  float* b = out + YH_POINT_BSDF;
  put3(YH_POINT_BSDF, sb.diffuse), put3(YH_POINT_BSDF + 3, sb.specular), put3(YH_POINT_BSDF + 6, sb.metal);
  put3(YH_POINT_BSDF + 9, sb.transmission), put3(YH_POINT_BSDF + 12, sb.refraction);
  b[15] = sb.roughness, b[16] = sb.opacity;
  b[17] = sb.diffuse_pdf, b[18] = sb.specular_pdf, b[19] = sb.metal_pdf, b[20] = sb.transmission_pdf, b[21] = sb.refraction_pdf;
  put3(YH_POINT_DENSITY, ps.medium.density), put3(YH_POINT_SCATTER, ps.medium.scatter), out[YH_POINT_ANISOTROPY] = ps.medium.anisotropy;
}

// object, element: n; slot_of: the leaf slot of every element of the shapes the batch names, the elements of object k's shape from
// slot_base[k] on (k_point_slots below); uv, outgoing: 2n, 3n; slots: two float4 per row (the lane form's medium_mem)
template <int FORM, bool GENERAL>
__global__ __launch_bounds__(256) void YH_POINT_KERNEL(const yhd_scene sc, int n, const int* object, const int* element, const int* slot_of,
    const int* slot_base, const float* uv, const float* outgoing, yhd_float4* slots, float* out) {
  constexpr bool QUAD     = !YH_LANE;
  constexpr bool from_lds = FORM != 2 && !GENERAL;
  extern __shared__ v4f lds_dyn[];
  trace_ctx tc;
  tc.sc = &sc, tc.ls = nullptr, tc.sc_dev = nullptr, tc.stats = nullptr, tc.lds_stack = nullptr, tc.lds_once = nullptr;
  tc.lds_scene = nullptr, tc.lds_lights = nullptr, tc.lds_envtab = nullptr, tc.lds_mats = nullptr;
  if constexpr (from_lds) {  // the tables where a launch has them (dev_trace.h: stage_tables)
    YH_LDS float* lds_cam;
    stage_tables(sc, (YH_LDS v4f*)lds_dyn, threadIdx.x, blockDim.x, tc, lds_cam);
    __syncthreads();
  }
  int  i     = (int)(blockIdx.x * blockDim.x + threadIdx.x) >> (QUAD ? 2 : 0);
  bool valid = i < n;
  if (!valid) {
    if (!QUAD) return;
    i = n - 1;  // whole quads stay converged; surplus quads redo the last row
  }
  const size_t r = (size_t)i;
  hit_t        isec;
  isec.object = object[r], isec.slot = slot_of[slot_base[isec.object] + element[r]];
  isec.u = uv[2 * r], isec.v = uv[2 * r + 1], isec.distance = 0.0f;
  point_row<FORM, GENERAL>(tc, isec, ld3(outgoing + 3 * r), slots + 2 * r, valid && (!QUAD || (threadIdx.x & 3) == 0), out + YH_POINT_FLOATS * r);
}

#if !YH_LANE
// The leaf order of one shape inverted: every leaf record holds its element (a triangle's in [0].w, a segment's in [2].w), slot_of[element]
// = the record's place. object: one that has the shape; num: the shape's elements.
__global__ __launch_bounds__(256) void k_point_slots(const yhd_scene sc, int object, int num, int* slot_of) {
  const int slot = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (slot >= num) return;
  const yhd_object& o     = sc.objects[object];
  const bool        lines = o.kind == YH_KIND_LINES;
  const int element = __float_as_int(lines ? sc.prims[(size_t)o.prim_base + (size_t)slot * 4 + 2].w : sc.prims[(size_t)o.prim_base + (size_t)slot * 6].w);
  if ((unsigned int)element < (unsigned int)num) slot_of[element] = slot;
}
extern "C" int yhk_point_slots(const yhd_scene* sc, int object, int num, int* slot_of, hipStream_t s) {
  if (num < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_point_slots, dim3((num + 255) / 256), dim3(256), 0, s, *sc, object, num, slot_of);
  return (int)hipGetLastError();
}
#endif

template <int FORM, bool GENERAL>
static int point_launch(const yhd_scene* sc, int n, const int* object, const int* element, const int* slot_of, const int* slot_base, const float* uv,
    const float* outgoing, void* slots, float* out, hipStream_t s) {
  const int lds = (FORM != 2 && !GENERAL) ? YHD_LDS_TABLES_F4(sc) * 16 : 0;
  auto      k   = YH_POINT_KERNEL<FORM, GENERAL>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
  }
  const int rows_per_block = YH_LANE ? 256 : 64;
  hipLaunchKernelGGL(k, dim3((n + rows_per_block - 1) / rows_per_block), dim3(256), lds, s, *sc, n, object, element, slot_of, slot_base, uv, outgoing,
      (yhd_float4*)slots, out);
  return (int)hipGetLastError();
}

// form: 0 / 2 in the quad unit, 1 in the lane unit; the scene's variant as a launch settles it (yhk_trace, yhk_stream)
extern "C" int YH_POINT_LAUNCH(const yhd_scene* sc, int form, int n, const int* object, const int* element, const int* slot_of, const int* slot_base,
    const float* uv, const float* outgoing, void* slots, float* out, hipStream_t s) {
  if (n < 1) return (int)hipErrorInvalidValue;
  const bool general = sc->general_materials != 0;
#if YH_LANE
  if (form != 1) return (int)hipErrorInvalidValue;
  return general ? point_launch<1, true>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s)
                 : point_launch<1, false>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s);
#else
  if (form == 0)
    return general ? point_launch<0, true>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s)
                   : point_launch<0, false>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s);
  if (form != 2) return (int)hipErrorInvalidValue;
  return general ? point_launch<2, true>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s)
                 : point_launch<2, false>(sc, n, object, element, slot_of, slot_base, uv, outgoing, slots, out, s);
#endif
}
