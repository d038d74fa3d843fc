/*
 * yhair.h — C ABI of the MI355X-native hair path-tracing sample loop.
 *
 * This is the drop-in boundary for the ONE hot path of dsforza96/yocto-hair:
 *   trace_samples -> trace_sample -> trace_path -> {BVH traversal, ray-line /
 *   ray-triangle intersection, hair BSDF eval / sample / pdf, light MIS}.
 *
 * The reference has no FFI layer. The narrowest seam it has is the
 * yocto::pathtrace C++ API (libs/yocto_pathtrace/yocto_pathtrace.h:207-230:
 * init_bvh, init_lights, init_state, trace_samples) and, one level down, the
 * four yocto::extension functions (libs/yocto_extension/yocto_extension.h:
 * 115-125). Every entry point below names the reference interface it replaces.
 *
 * Conventions: plain C types only, no exceptions cross the boundary. Every
 * function returning int returns YH_OK (0) on success or a negative YH_E_*
 * code; yh_last_error() gives the text. Host arrays passed in are borrowed for
 * the duration of the call only. A context owns all of its device memory and
 * is bound to ONE GPU (one process per GPU is the deployment model; image
 * tiles are sharded across processes with yh_set_shard()).
 *
 * All vectors are packed floats; frames are 12 floats x,y,z,o column vectors
 * exactly as yocto::math::frame3f (libs/yocto/yocto_math.h, frame3f).
 */
#ifndef YHAIR_H_
#define YHAIR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YH_OK 0
#define YH_E_INVALID -1     /* bad argument / unsupported scene feature      */
#define YH_E_DEVICE -2      /* HIP runtime error (no GPU, launch failure...) */
#define YH_E_STATE -3       /* call order violated (e.g. trace before init)  */
#define YH_E_IO -4          /* file not found / parse error                  */
#define YH_E_SELFTEST -5    /* a Monte-Carlo self-test left its tolerance    */

/* ------------------------------------------------------------------------ */
/* Scene description (geometry level, no acceleration data).                 */
/* Mirrors the subset of yocto::pathtrace scene structs reachable from the   */
/* hair path (yocto_pathtrace.h:272-387).                                    */
/* ------------------------------------------------------------------------ */

/* ptr::shape (yocto_pathtrace.h:335-366). Exactly one of lines / triangles
 * is non-empty. For line shapes `normals` holds the hair TANGENTS
 * (yocto_pbrt.h:1782-1787) and `radius` must be given.                      */
typedef struct yh_shape {
  int          num_vertices;
  const float* positions; /* 3 * num_vertices                              */
  const float* normals;   /* 3 * num_vertices, or NULL                     */
  const float* radius;    /* num_vertices, or NULL (triangles)             */
  int          num_lines;
  const int*   lines;     /* 2 * num_lines                                 */
  int          num_triangles;
  const int*   triangles; /* 3 * num_triangles                             */
  const float* texcoords; /* 2 * num_vertices, or NULL (texcoord = element uv,
                             yocto_pathtrace.cpp:295-311)                   */
} yh_shape;

/* A colour texture (ptr::texture colorf / colorb, yocto_pathtrace.h:282-287):
 * RGB, row-major, top row first. Byte textures are sRGB-encoded unless the
 * lookup asks for linear (lookup_texture, yocto_pathtrace.cpp:147-164).      */
typedef struct yh_texture {
  int         width, height;
  int         is_byte; /* 1: pixels = uint8 RGB (colorb); 0: float RGB (colorf) */
  const void* pixels;
} yh_texture;

/* ptr::material (yocto_pathtrace.h:293-329), restricted to the lobes the hair
 * configs reach: emission, diffuse colour and the hair parameters
 * (yocto_extension.h:86-95). Specular, metallic, transmission / refraction,
 * delta (roughness 0) and opacity lobes follow yocto_pathtrace.cpp:405-471,
 * homogeneous volumes :498-533,1403-1414,1458-1497. The colour textures are
 * here (emission_tex, color_tex, scattering_tex: 1-based index into
 * yh_scene_desc::textures, 0 = none); the scalar and normal maps of the same
 * material are in a yh_material_maps of its own (yh_upload_scene_maps), so
 * that this struct keeps its layout.                                         */
typedef struct yh_material {
  float emission[3];
  float color[3];
  float specular, metallic, roughness, transmission, opacity, ior;
  int   thin;
  float sigma_a[3];
  float beta_m, beta_n, alpha, eta, eumelanin, pheomelanin;
  /* homogeneous volume inside a closed surface (thin = 0 and transmission > 0,
   * yocto_pathtrace.cpp:498-533): density = -log(clamp(color, 1e-4, 1)) / trdepth */
  float scattering[3];
  float scanisotropy;
  float trdepth;      /* 0.01 (yocto_pathtrace.h:305)                          */
  int   emission_tex, color_tex, scattering_tex; /* 1-based, 0 = none          */
} yh_material;

/* The scalar and normal maps of a material (ptr::material, yocto_pathtrace.h:
 * 311-320): 1-based index into yh_scene_desc::textures, 0 = none. Every map is
 * looked up linear (bytes / 255, no sRGB decode) with the bilinear wrap lookup
 * of the colour textures at the hit's texture coordinates. A scalar texture is
 * passed as a grey RGB one: lookup_texture treats both alike (pt.cpp:147-164). */
typedef struct yh_material_maps {
  int specular_tex;     /* specular  *= eval_texture(specular_tex).x    (pt.cpp:413-414) */
  int metallic_tex;     /* metallic  *= eval_texture(metallic_tex).x    (pt.cpp:415-416) */
  int roughness_tex;    /* roughness *= eval_texture(roughness_tex).x   (pt.cpp:417-418), squared after */
  int transmission_tex; /* read by no lookup: transmission is scaled by emission_tex (pt.cpp:421-422);
                           checked and otherwise ignored                                             */
  int opacity_tex;      /* opacity   *= mean(eval_texture(opacity_tex)) (pt.cpp:423-424), hair included */
  int normal_tex;       /* eval_normalmap (pt.cpp:329-347): triangle shapes only (pt.cpp:350-369)    */
} yh_material_maps;

/* ptr::object (yocto_pathtrace.h:369-373) */
typedef struct yh_object {
  float frame[12];
  int   shape;
  int   material;
} yh_object;

/* ptr::environment (yocto_pathtrace.h:376-380); texels = linear float RGB,
 * row-major, top row first, or NULL for a constant environment.             */
typedef struct yh_environment {
  float        frame[12];
  float        emission[3];
  int          tex_width, tex_height;
  const float* texels;
} yh_environment;

/* ptr::camera (yocto_pathtrace.h:272-278) */
typedef struct yh_camera {
  float frame[12];
  float lens;
  float film[2];
  float focus;
  float aperture;
} yh_camera;

typedef struct yh_scene_desc {
  int                   num_shapes;
  const yh_shape*       shapes;
  int                   num_materials;
  const yh_material*    materials;
  int                   num_objects;
  const yh_object*      objects;      /* in reference order (alphabetical)  */
  int                   num_environments;
  const yh_environment* environments;
  yh_camera             camera;
  int                   num_textures; /* material textures (environments carry their own) */
  const yh_texture*     textures;
} yh_scene_desc;

/* shader_type (yocto_pathtrace.h:177-182), same values as the reference's enum */
enum {
  YH_SHADER_NAIVE    = 0, /* trace_naive    (pt.cpp:1514-1581): brdf sampling only, no MIS, no volumes */
  YH_SHADER_PATH     = 1, /* trace_path     (pt.cpp:1380-1511): the hot path                            */
  YH_SHADER_EYELIGHT = 2, /* trace_eyelight (pt.cpp:1584-1641): light at the eye, delta chains only     */
  YH_SHADER_NORMAL   = 3, /* trace_normal   (pt.cpp:1644-1658): shading normal as a colour              */
  YH_SHADER_COUNT    = 4
};

/* trace_params (yocto_pathtrace.h:188-197). NOTE: a zeroed struct selects
 * shader 0 = naive, as a zeroed reference trace_params would; fill `shader`. */
typedef struct yh_trace_params {
  int      resolution; /* 720                                               */
  int      bounces;    /* 8                                                 */
  float    clamp;      /* 100                                               */
  uint64_t seed;       /* 961748941                                         */
  int      shader;     /* YH_SHADER_PATH; others: "sampler unknown" error   */
  int      hair_exact; /* extension (0 = default). The hair BSDF is evaluated within 1e-4 relative of the
                        * reference with hardware reciprocal / sqrt / log2 / sin / cos and float asinf; 1 selects
                        * the exact forms (IEEE divisions, library log / sin / cos, the reference's DOUBLE asin,
                        * yocto_extension.cpp:111,148-151): paths follow the reference's for more bounces at about
                        * 0.88 x the speed. Path shader only; runs the 512 x 4 quad kernel (csrc/exact.hip).        */
} yh_trace_params;

/* Per-sample work counters of the reference algorithm: what
 * the roofline's algorithmic-bytes figure is built from.                    */
typedef struct yh_workcounts {
  uint64_t samples;
  uint64_t rays;       /* scene-level intersect calls                       */
  uint64_t nodes;      /* bvh_node visits: scene + shape + instance BVHs    */
  uint64_t seg_tests;  /* intersect_line calls                              */
  uint64_t tri_tests;  /* intersect_triangle calls                          */
  uint64_t hair_shades;
  uint64_t surf_shades;
  uint64_t env_lookups;
  uint64_t env_samples;
  /* wave-level profile of the instrumented launch (diagnostics): shader-clock
   * cycles in traversal / shading summed over waves, 100 MHz ticks spent on
   * tiles, regeneration-loop iterations, traversal trip counts per wave (max
   * over lanes) and per lane (sum), live lanes per iteration                 */
  uint64_t cyc_trace, cyc_shade, ticks_tile, wave_iters, wave_steps, lane_steps, lane_iters;
  uint64_t cyc_geom, cyc_sample, cyc_eval, cyc_rest; /* split of cyc_shade */
  /* divergence of the traversal loop: (wave trips that ran the code, lanes
   * active in them) for wide-node, line-leaf, triangle-leaf, ENTER and
   * scene-node steps                                                         */
  uint64_t branch[10];
} yh_workcounts;

typedef struct yh_context yh_context;

/* ------------------------------------------------------------------------ */
/* Context                                                                    */
/* ------------------------------------------------------------------------ */

/* Creates a context on HIP device `device`. Returns NULL when no usable GPU
 * or the HIP code object is missing: there is NO CPU fallback.
 * Every call that waits for the device waits at most YHAIR_LAUNCH_TIMEOUT_S seconds (environment, default 1800; this and every other
 * YHAIR_* variable the library reads: the table at the head of yocto-hair_amd/host/switches.h): a launch that
 * does not complete in time returns YH_E_DEVICE, and from then on the context refuses every call that would touch the device
 * (a hung kernel cannot be recalled); yh_destroy of such a context returns at once and frees nothing. A caller that wants to
 * retry starts a fresh process. (The reference's trace_samples cannot hang: CPU threads over rows, yocto_pathtrace.cpp:1954-1989.) */
yh_context* yh_create(int device);
void        yh_destroy(yh_context* ctx);
/* Text of the last error on this context (or of the failed yh_create when
 * ctx == NULL). Never NULL.                                                 */
const char* yh_last_error(const yh_context* ctx);
/* Library version string and the code-object architecture it was built for. */
const char* yh_version(void);

/* ------------------------------------------------------------------------ */
/* Whole-path API: replaces yocto::pathtrace                                  */
/* ------------------------------------------------------------------------ */

/* init_bvh + init_lights (yocto_pathtrace.cpp:755-818, 1695-1740): builds the
 * two-level BVH (reference-identical binary middle-split tree, so that
 * closest-hit results, including exact-t ties, match the reference), the
 * area-light triangle CDFs and the environment texel CDF, precomputes inverse
 * object frames and per-material hair constants, and uploads everything. Shapes of 32 768 primitives and more are built ON THE
 * DEVICE from their vertex arrays as they are (bounds, tree, leaf-ordered records), and every shape's tree is collapsed there into
 * the 4- / 8- / 16-wide nodes the kernels traverse (csrc/bvh_gpu.hip): the call returns with everything a launch will read in
 * place (1.6 M hair segments: 41 ms); the host arrays are borrowed for the call only.
 * LIMITS (YH_E_INVALID with a message beyond them): a shape holds fewer than 2^27 elements; the traversal kernels address a
 * scene's trees as one array of 32-byte units with 27-bit leaf references and 30-bit node references — a line segment takes one
 * unit, a triangle two, a 4- / 8- / 16-wide node four / eight / sixteen — i.e. about 134 M segments or 67 M triangles in ALL shapes together (instances share
 * their shape); at most 4 environments and 16 lights (every object with an emissive material is one, so every instance of an emitter
 * is). Scenes of more than ~46 objects or 24 materials run the GENERAL
 * kernel variants (their tables do not fit the LDS budget): slower, same pixels. The scene level of a scene of more than ~46 objects
 * — what an instanced scene file expands to — is collapsed like a shape's tree, two levels per node, and walked as 4-wide nodes out of the same
 * array, in the reference's visiting order: four more units per scene node, about a third of a node per object (4096 objects: ~1 400
 * nodes) — and the upload RESERVES four units per OBJECT there (a wide node stands for an internal node of the binary tree, of which
 * a tree over n objects has at most n - 1), so that yh_update_objects can write the nodes of any tree over the same objects; the
 * reservation is what counts in the limits above. The one-lane kernels (the streaming integrator
 * of dense hair, large closest-hit batches) address that array with 32-bit byte offsets: beyond 4 GB of it (about fifty million
 * segments) they are not candidates and the quad kernels render — same pixels.                                                */
int yh_upload_scene(yh_context* ctx, const yh_scene_desc* scene);
/* The same with the materials' scalar and normal maps: `maps` holds scene->num_materials entries, or is NULL
 * (yh_upload_scene(ctx, scene) is yh_upload_scene_maps(ctx, scene, NULL)). A material with a specular, metallic,
 * roughness, opacity or normal map runs the GENERAL kernel variants, which look its maps up at every hit. An index
 * outside [0, num_textures] is YH_E_INVALID and leaves the context's previous scene as it was.                     */
int yh_upload_scene_maps(yh_context* ctx, const yh_scene_desc* scene, const yh_material_maps* maps);

/* EDITS OF THE UPLOADED SCENE that leave every shape's acceleration structure as it is (yh_update_shape, further down, builds ONE
 * shape's again). The reference reads its scene structs live: its
 * interactive caller edits app->camera->frame in place and the next sample uses it (apps/ysceneitraces/ysceneitraces.cpp:392-410).
 * Here the description was flattened by yh_upload_scene, so an edit is a call:
 *   yh_update_camera        set_frame / set_lens / set_focus on a camera (yocto_pathtrace.h:97-104): the whole yh_camera;
 *   yh_update_materials     the material setters (yocto_pathtrace.h:106-140): rows [first, first + count) of the material table,
 *                           `materials` holding `count` entries;
 *   yh_update_environments  set_frame / set_emission on an environment (yocto_pathtrace.h:172-174): frame and emission of every
 *                           environment; count must be the uploaded scene's num_environments; tex_width, tex_height and texels
 *                           are ignored (the texel cdf depends on neither the emission scale nor the frame);
 *   yh_update_objects       set_frame / set_material on an object (yocto_pathtrace.h:110-111): rows [first, first + count) of the
 *                           object list, `objects` holding `count` entries. Shape trees live in object space, so no shape is touched:
 *                           the rows' inverse frames and world boxes are made on the device, one lane per row, with the upload's own
 *                           arithmetic (unit/objects.hip), the reference's scene-level tree over ALL world boxes is built again as the
 *                           upload builds it, and with it the scene-level table sizes, the 4-wide scene nodes at the front of the
 *                           traversal array (scenes of more than ~46 objects) and the stack depths.
 * CONTRACT. After a successful call the context is, for every later call, indistinguishable in its results from a context that got
 * yh_upload_scene_maps of the edited description: pixels, RNG states, yh_lights_batch, yh_intersect_batch, yh_intersect_plain_batch and
 * yh_scene_once are the same bits (the kernel variant, the once-per-ray form and the fingerprint of the kernel-trial record follow the
 * edit). The image state is gone, as after an upload: yh_trace_samples before a new yh_init_state returns YH_E_STATE, and that
 * yh_init_state probes and plans as for a new scene. The calls are blocking and need an uploaded scene (else YH_E_STATE). No device
 * work or allocation is proportional to the geometry: no shape's tree, record, vertex array or light cdf is read, written or
 * reallocated (1.6 M hair segments: an upload builds for 41 ms on the device alone, an edit copies a few hundred bytes);
 * yh_update_objects works and allocates in proportion to the number of OBJECTS.
 * REFUSED with YH_E_INVALID, a message that names the entry point, and the context exactly as it was (it goes on rendering the
 * earlier scene): a NULL argument (with count != 0); first / count outside the uploaded table; count != num_environments; a material
 * or environment whose emission changes between all-zero and not all-zero (the light list, init_lights,
 * yocto_pathtrace.cpp:1695-1740, depends on it and the shapes' host arrays were borrowed for the upload only) — and likewise an object
 * whose new material and uploaded one differ in that; a material whose emission_tex, color_tex or scattering_tex differs from the
 * uploaded one (which texel copies exist was decided at the upload); an object row whose shape differs from the uploaded row's or
 * whose material lies outside the uploaded table. Two refusals of yh_update_objects follow from the RESULT of the edit: the tree
 * over the moved objects is too deep for the traversal stack (the upload's "BVH too deep" check), or the scene level changes its
 * form between the kernels' LDS table and 4-wide nodes in the traversal array (the table's size counts the scene tree's nodes, so a
 * scene of about 45 objects can cross the 10 KB line by moving them): room for wide scene nodes exists only where the upload put it,
 * and the answer is a new upload. The materials' maps (yh_material_maps) are not editable. A HIP error once an edit has begun to
 * write returns YH_E_DEVICE and leaves the context without a scene, as a failed upload does.
 * OUT OF SCOPE, for all of which the answer stays a new upload: changing an object's shape, adding or removing objects or shapes,
 * changing a shape's counts, the geometry of an emitter, textures and maps, turning emission on or off. (Vertex edits that keep a
 * shape's counts: yh_update_shape, below. What changes the light list — emission on or off, an emitter's geometry — is an edit after
 * yh_set_light_edits: LIGHT EDITS, below.)                                                                                         */
int yh_update_camera(yh_context* ctx, const yh_camera* camera);
int yh_update_materials(yh_context* ctx, int first, int count, const yh_material* materials);
int yh_update_environments(yh_context* ctx, int count, const yh_environment* environments);
int yh_update_objects(yh_context* ctx, int first, int count, const yh_object* objects);

/* VERTEX EDITS OF ONE SHAPE: set_positions / set_normals / set_radius on a shape followed by init_bvh (yocto_pathtrace.h:154-157) —
 * a groom being combed, a simulation step, a strand-width sweep. `now` is the whole shape `shape` of the uploaded list, borrowed
 * for the call: num_vertices, num_lines and num_triangles must equal the uploaded shape's; normals and texcoords must be present or
 * absent as at the upload; radius may be given or NULL, as at an upload (NULL: 0.001); the index array is read again, so another
 * topology with the same counts is an edit too.
 *   yh_update_shape         the arrays are HOST arrays;
 *   yh_update_shape_device  every non-NULL pointer of `now` is a DEVICE pointer on the context's GPU (e.g. the data_ptr() of a
 *                           contiguous float32 / int32 torch tensor): the vertices of a GPU simulation never visit the host. The
 *                           call runs on the context's own non-blocking stream and returns when done: earlier writes to the arrays
 *                           from other streams (e.g. a torch kernel that deforms them) must have completed before.
 * The CONTRACT above holds for both: afterwards pixels, RNG states, yh_lights_batch, yh_intersect_batch, yh_intersect_plain_batch,
 * yh_scene_once and the kernel-trial fingerprint are those of a context that got yh_upload_scene_maps of the edited description, and
 * the image state is gone. The edited shape's bounds, the reference's tree, its leaf and test records, its 4- / 8- / 16-wide nodes
 * and its per-vertex rows are made again with the upload's own code — on the device for shapes of 32 768 primitives and more (and
 * always in the device form), on the host for smaller ones, the upload's rule — and from its new root box the world boxes of the
 * objects that name it and the scene level, as after yh_update_objects. Work and allocation are proportional to the edited shape and
 * to the number of objects: no other shape's records or nodes, no texture, environment cdf or light table is touched.
 * ROOM. The number of a shape's wide nodes depends on its positions. An upload gives every shape exactly the room its nodes take.
 * An edit whose 4-, 8- and 16-wide nodes fit the shape's room writes them in place (the unused rest is zero). A width that does not
 * fit gets a new region behind the end of the traversal array, on a multiple of 4 units, with room for count + count / 8 nodes; the
 * array is allocated again and its bytes copied device to device, unchanged; the vacated region is zeroed and NOT reused: a fresh
 * upload reclaims it. No other shape moves. The 30-bit unit limit of yh_upload_scene holds for the grown array, and the one-lane
 * kernels' 4 GB candidacy follows it (their 32-bit offsets must reach the furthest 4-wide region).
 * REFUSED with YH_E_INVALID, a message that names the entry point, and the context exactly as it was: a NULL `now`; `shape` outside
 * the uploaded list; a count that differs; lines against triangles; normals or texcoords present where the upload had none or the
 * reverse; NULL positions; a vertex index outside [0, num_vertices) (found by a kernel before anything follows an index, in both
 * forms); a shape named by an object whose material emits (the light cdf and the kernels' light table are made from it); a tree too
 * deep for the traversal stack; yh_update_objects' two refusals (the scene level changes its form, or needs more wide scene nodes
 * than the upload left room for); the 30-bit limit. YH_E_STATE before an upload. A HIP error once the edit has begun to write
 * returns YH_E_DEVICE and leaves the context without a scene.                                                                      */
int yh_update_shape(yh_context* ctx, int shape, const yh_shape* now);
int yh_update_shape_device(yh_context* ctx, int shape, const yh_shape* now);
/* REFIT: the same vertex edit, kept in the tree the shape HAS — a simulation step, a comb stroke, a sway, in which strands move a
 * fraction of their length. Arguments, borrowing, stream rules and refusals are those of yh_update_shape / _device (the whole yh_shape:
 * the index array is read again, records are made from idx[element], and any primitives are valid under recomputed boxes). Nothing is
 * built: every leaf slot keeps its element (the record in it holds the element id) and is written again from the new arrays, the
 * bits the upload's leaf records have; the test records are made from them; the boxes of the shape's 4-, 8- and 16-wide nodes are
 * recomputed bottom-up in place — a leaf slot's the union of its primitives' line_bounds / triangle_bounds (radius 0.001 where the
 * shape has none), an internal slot's the union of the child node's slots, an empty slot's stays; references, axes and occupied bits
 * are not written — one kernel launch per level of each wide tree, deepest first (no boxes pass between workgroups inside a launch);
 * the per-vertex rows are written again; the root box, the rows and world boxes of the objects that name the shape and the scene
 * level follow as after yh_update_shape (the reference's scene-level tree is built exactly: it is cheap). The traversal array neither
 * grows nor moves (yh_shape_nodes reports the same offsets, counts and room), the stack depths stay, no other shape's bytes are
 * touched, and the only scratch the shape sizes is its primitive boxes in leaf order (24 bytes each) and the host form's staged arrays.
 * Everything that can refuse — the checks, the index check by kernel, the new root box (a min / max reduction, exact and order-free)
 * and the scene level's two refusals — runs before the first write: a refused call leaves the context exactly as it was.
 * CONTRACT. After yh_refit_shape the context holds a valid tree over the edited description with the topology of the shape's last
 * BUILD (the upload, or the last yh_update_shape). Closest hits are those of a fresh upload: the distance of every ray is the same
 * bits; object, element and uv are the same except where two primitives lie at bit-equal closest distance — the winner of such a
 * tie follows the visiting order, which is the old topology's. Images are therefore those of a fresh upload except on paths that
 * meet such a tie. Where the edited description has the same reference tree as the last build (a uniform scale by two, an edit of
 * tangents, radii or texcoords that moves no centre across a split), EVERYTHING is the same bits as after a fresh upload. Render
 * speed after large deformations degrades, because boxes overlap: the caller's trade. yh_update_shape with the same arrays restores
 * the reference's tree, and with it bit-for-bit identity with a fresh upload in every case.
 * yh_shape_refit_growth is the number to make that trade with: per width (4, 8, 16) the sum of the half-areas of all occupied slot
 * boxes of the shape's nodes NOW over the same sum at the shape's last build, summed on the device in double in a fixed order:
 * exactly 1.0f after an upload, after yh_update_shape and after a refit that reproduces the boxes. YH_E_STATE before an upload.     */
int yh_refit_shape(yh_context* ctx, int shape, const yh_shape* now);
int yh_refit_shape_device(yh_context* ctx, int shape, const yh_shape* now);
int yh_shape_refit_growth(const yh_context* ctx, int shape, float growth[3]);
/* A diagnostic: where shape `shape`'s 4-, 8- and 16-wide nodes sit in the traversal array (offset, in 32-byte units), how many
 * nodes it has of each width (count) and how many its region has room for (room). YH_E_STATE before an upload.                    */
int yh_shape_nodes(const yh_context* ctx, int shape, int64_t offset[3], int count[3], int room[3]);

/* LIGHT EDITS: muting or soloing a light, handing an object an emitter's material, reshaping an emitting mesh. Off by default: every
 * paragraph above holds as written. yh_set_light_edits(ctx, 1) — any time, before or after an upload; YH_OK — REPLACES, in seven entry
 * points, the refusal of an edit merely because it changes the light list (init_lights, yocto_pathtrace.cpp:1695-1740):
 *   yh_update_materials, yh_update_environments   "turns its emission on / off: the light list changes";
 *   yh_update_objects                             "object turns its emission on / off with material";
 *   yh_update_shape, yh_update_shape_device,
 *   yh_refit_shape, yh_refit_shape_device         "is the shape of object, whose material emits: the light tables are made from it".
 * Such an edit makes the light list again by the upload's rule: objects first, in order — an object is a light when its material's
 * emission is not all zero and its shape has triangles (a line shape never is one; every instance of an emitter is a light of its own)
 * — then the environments, in order; every light has its segment of the light cdf; a light of at most 4 triangles has its record in the
 * kernels' LDS light table, a larger one is read through memory and selects the GENERAL kernel variant; the first textured environment
 * light of at least 4096 texels gets the coarse index of its cdf. A light that appears in the middle shifts every later light's index.
 * The CONTRACT of the edits holds unchanged: pixels, RNG states, yh_lights_batch, yh_intersect_batch, yh_intersect_plain_batch,
 * yh_scene_once, the kernel variant and the kernel-trial fingerprint are those of a context that got yh_upload_scene_maps of the edited
 * description (after a REFIT: ties apart, as above — the cdf is by element and does not depend on the tree), and the image state is gone.
 * The list is made where its data is (unit/light_list.hip), from the vertex and index rows, leaf records and root boxes the context
 * keeps on the device: a triangle's area is the upload's arithmetic, the cdf ONE float chain in element order inside one wavefront per
 * light (no reordered sum gives the upload's bits), all lights in one launch. After a vertex edit of an emitter's shape the cdf and the
 * record of every light that names it are written again where they are, from the new arrays as they sit on the device: nothing is read
 * back, no other light, shape or environment cdf is touched, and the work is proportional to that emitter's triangles. A textured environment's texel cdf uses the host's sine and is never computed on
 * the device: a light that exists keeps its segment (a device-to-device copy); one that did not emit at the upload gets its cdf when
 * it first turns on, made by the upload's own loop from the texels the device kept (the caller passes none), and the context keeps it:
 * off and on again costs a copy.
 * STILL REFUSED with YH_E_INVALID, a message that names the entry point, and the context exactly as it was: an edit that would make
 * more than 16 lights (the message names the object); one that would leave the scene without a light; a changed emission_tex,
 * color_tex or scattering_tex; and every argument, count, depth and scene-level refusal of the entry points above. Everything that can
 * refuse runs before the first write; a HIP error after it returns YH_E_DEVICE and leaves the context without a scene. Another
 * environment texture, textures and maps, counts and new objects stay an upload.                                                     */
int yh_set_light_edits(yh_context* ctx, int on);
/* A diagnostic: lights[] of the uploaded scene in the kernels' order: per light the object (-1: an environment), the environment (-1:
 * an object), the cdf entries, and whether its record is in the LDS light table. Returns the number of lights and fills at most
 * `capacity` entries of every non-NULL array. YH_E_STATE before an upload.                                                           */
int yh_light_list(const yh_context* ctx, int* object, int* environment, int* cdf_count, int* in_lds, int capacity);
/* init_lights' area cdf of one triangle shape (yocto_pathtrace.cpp:1695-1740): cdf[t] = area[t] + cdf[t - 1], one float chain in
 * element order. yh_triangle_cdf: the host's restatement (no GPU, no context); yh_triangle_cdf_gpu: the kernel of the light edits.
 * Same bits. YH_E_INVALID: a NULL array, no vertices or triangles, an index outside the vertices.                                     */
int yh_triangle_cdf(int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf);
int yh_triangle_cdf_gpu(yh_context* ctx, int num_vertices, const float* positions, int num_triangles, const int* triangles, float* cdf);

/* init_state (yocto_pathtrace.cpp:1931-1946): image size from the camera film
 * and params->resolution, zeroed accumulators, per-pixel PCG32 streams
 * make_rng(seed, rand1i(master, 1<<31)/2+1) with master = make_rng(1301081). */
/* On an image this context has not rendered yet it also launches a 1-sample
 * PROBE of the path shader (the per-tile costs that plan the first real launch)
 * and puts accumulators and RNG streams back as they were: blocking, one
 * kernel launch, no effect on the pixels.                                     */
int yh_init_state(yh_context* ctx, const yh_trace_params* params);
int yh_image_size(const yh_context* ctx, int* width, int* height);

/* Tile sharding for one-process-per-GPU rendering: this
 * context renders only the 8x8-pixel tiles with tile_id % world == rank.
 * Pixel results do not depend on (rank, world). Call before yh_init_state.   */
int yh_set_shard(yh_context* ctx, int rank, int world);

/* trace_samples called `nsamples` times (yocto_pathtrace.cpp:1992-2007, call
 * site apps/yscenetrace/yscenetrace.cpp:256-258): adds nsamples samples to
 * every owned pixel. Blocking. Normally one kernel launch; a request of 64
 * samples or more on an image whose kernels have not been timed yet starts
 * with 32-sample launches of the candidates (same samples, same bits:
 * yh_last_trace_ms reports the sum and the number of launches): up to three
 * kernels, each tried once, twice when two of them tie within 15 %.          */
int yh_trace_samples(yh_context* ctx, int nsamples);
/* Same, but only enqueues the work on the context's stream.                  */
int yh_trace_samples_async(yh_context* ctx, int nsamples);
int yh_synchronize(yh_context* ctx);

/* state->render (yocto_pathtrace.h:426-429): accumulated / samples, float4
 * per pixel, row-major top row first. Non-owned pixels are 0.                */
int yh_download(yh_context* ctx, float* rgba);
/* tonemap + float_to_byte (yocto_math.h:3820-3829, 3721-3729), the last step of the interactive caller's reset_display
 * (apps/ysceneitraces/ysceneitraces.cpp:280,296), on the device: accumulated / samples, scaled by exp2(exposure) when
 * exposure != 0, through the fitted ACES curve (yocto_math.h:3788-3794) when `filmic`, through rgb_to_srgb when `srgb`,
 * then clamp(int(a * 256), 0, 255) per channel — alpha too, which no curve touches. rgba8: four bytes per pixel (r, g, b, a),
 * row-major top row first; non-owned pixels are 0 and a non-finite value gives 0. Blocking; YH_E_STATE before yh_init_state.   */
int yh_download_display(yh_context* ctx, float exposure, int filmic, int srgb, uint8_t* rgba8);
/* Packs the owned tiles' float4 pixels into a DEVICE buffer (the payload of
 * the RCCL gather). `capacity` in float4 pixels; *count receives the number
 * written. Tiles are in increasing tile_id order, 64 pixels per tile. This
 * call and yh_unpack_tiles_device run on the context's own non-blocking
 * stream and return when done: earlier writes to the buffers from other
 * streams (e.g. a torch allocation's fill) must have completed before.       */
int yh_pack_tiles_device(yh_context* ctx, void* device_rgba, int64_t capacity,
    int64_t* count);
/* Inverse on the gathering rank: scatters rank `src_rank`'s packed tiles into
 * a full W*H float4 DEVICE image.                                            */
int yh_unpack_tiles_device(yh_context* ctx, const void* device_packed,
    int src_rank, int world, void* device_image);
/* Number of float4 pixels yh_pack_tiles_device writes for (rank, world).     */
int64_t yh_shard_pixels(const yh_context* ctx, int rank, int world);

/* Multi-GPU inside ONE process (yscenetrace --gpus N; the reference renders on one device and has
 * no counterpart, the seam is save_image's input, apps/yscenetrace/yscenetrace.cpp:270): `n`
 * contexts, context i holding shard (i, n) of the same image (yh_set_shard) and the same number of
 * samples. Every context packs its tiles; ONE ncclGather over RCCL / xGMI (grouped, one call per
 * communicator; librccl is opened on first use) brings them to contexts[0], which un-interleaves
 * them and copies the full W*H float4 image to `rgba`. Contexts that share a device (tests on a
 * one-GPU box) or YHAIR_GATHER=peer use device-to-device copies instead of the collective.        */
int yh_gather_framebuffer(yh_context** contexts, int n, float* rgba);

/* Per-pixel state (yocto_pathtrace.h:419-423) for checkpoint / parity tests:
 * rng state words (2 x u64 per pixel) and sample count.                      */
int yh_download_rng(yh_context* ctx, uint64_t* state_inc);

/* FIRST-HIT FEATURE PASS (an extension: the reference has no counterpart). Per pixel of the image of yh_init_state, the camera
 * ray's first intersection (intersect_scene_bvh, as yh_intersect_batch) and what the `normal` shader evaluates at it (trace_normal,
 * yocto_pathtrace.cpp:1644-1658: eval_position, eval_normal with the normal map, the orthonormalised normal of a line and the flip of
 * a thin material; no opacity pass-through). One plane per quantity, row-major top row first, one entry per pixel; a NULL plane is
 * skipped with, where possible, the work behind it; at least one must be given.
 *   plane               type     hit                                                            miss
 *   object, element     int      the hit's object and element                                   -1
 *   material            int      the object's material                                          -1
 *   uv                  float2   element uv of the hit                                          0
 *   distance            float    ray distance                                                   0
 *   position            float3   eval_position (a strand: on its axis)                          0
 *   normal              float3   the shading normal described above                             0
 *   tangent             float3   eval_normal of a line hit (strand direction); 0 on triangles   0
 *   texcoord            float2   eval_texcoord                                                  0
 *   albedo              float3   material colour x colour texture (:411-412), hair included      0
 *   ray                 6 float  origin, direction of the traced ray                            the same
 * mode YH_GBUFFER_CENTRE: the pinhole ray through the pixel centre (sample_camera at uv + 0.5 with the lens point at zero whatever
 * the aperture): guides that depend neither on depth of field nor on the render's progress. YH_GBUFFER_NEXT_SAMPLE: the ray the
 * pixel's NEXT sample will take, drawn from a copy of its stream (nothing is written back): with the `normal` shader the next
 * yh_trace_samples(1) adds exactly normal * 0.5 + 0.5 to a hit pixel.
 * The pass covers the WHOLE image on every context, whatever yh_set_shard says, so a multi-GPU caller runs it on one context and needs
 * no gather; it costs about one sample of the `normal` shader. It changes no accumulator, stream, sample count, trial record or launch
 * shape: a render interleaved with it has the bits it has without it. Blocking; yh_last_trace_ms reports the kernel's event time.
 * yh_trace_gbuffer takes HOST pointers, yh_trace_gbuffer_device DEVICE pointers (written on the context's own stream, nothing copied).
 * YH_E_STATE before yh_upload_scene / yh_init_state or with an asynchronous launch pending; YH_E_INVALID for an unknown mode, a NULL
 * `out`, no plane at all, or a scene whose trees exceed the one-lane kernels' 32-bit offsets (4 GB).                                   */
#define YH_GBUFFER_CENTRE 0
#define YH_GBUFFER_NEXT_SAMPLE 1
typedef struct yh_gbuffer {
  int*   object;
  int*   element;
  int*   material;
  float* uv;
  float* distance;
  float* position;
  float* normal;
  float* tangent;
  float* texcoord;
  float* albedo;
  float* ray;
} yh_gbuffer;
int yh_trace_gbuffer(yh_context* ctx, int mode, const yh_gbuffer* out);
int yh_trace_gbuffer_device(yh_context* ctx, int mode, const yh_gbuffer* out);

/* DENOISE (an extension: the reference has no counterpart; the consumer of the feature pass above). An edge-avoiding a-trous wavelet
 * filter (Dammertz et al. 2010) over the resolved render, guided by the CENTRE-mode planes object, normal, position and albedo.
 * Per pixel p: colour c (float4), id (-1: a miss), normal n, position x, albedo a.
 *   effective albedo   per channel (a < 1e-3f) ? 1 : a; 1 when `demodulate` is 0, and 1 on a miss whatever the plane holds
 *   working colour     u = c.rgb / effective albedo; alpha is never filtered, the output's alpha is the input's
 *   level l            l = 0 .. iterations - 1, tap spacing s = 2^l, 25 taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner;
 *                      taps outside the image are skipped. h = k[|dx|] k[|dy|], k = {3/8, 1/4, 1/16};
 *                      w = h / (1 + x + 0.5 x x) — the reciprocal of exp's second-order Taylor polynomial, not exp(-x): + - x / and
 *                      comparisons only, so that device, host and a float32 restatement give the same bits — with
 *                      x = |n_p - n_q|^2 / sigma_normal^2 + |x_p - x_q|^2 / sigma_position^2 + |u_p - u_q|^2 / (sigma_color 2^-l)^2,
 *                      u the level's input; a term whose sigma is <= 0 contributes 0. w = 0 when `match_object` is set and the ids
 *                      differ, when a channel of u_q is not finite, when x >= 0 does not hold. One float accumulator per channel and
 *                      one for w, summed in tap order (a tap of weight 0 is not added): u'_p = sum w u_q / sum w, and u'_p = u_p
 *                      when the sum of w is 0 or u_p is not finite.
 *   misses             a pixel with id -1 passes every level unchanged: its output has its input's bits
 *   after the last     out.rgb = u x effective albedo. With iterations = 0 the output is the input.
 * It changes no accumulator, stream, sample count, item cost, trial record or launch shape. Blocking on the context's stream;
 * yh_last_trace_ms reports its kernels' event time and launch count (the feature pass included where the call runs it).
 * YH_E_STATE before yh_upload_scene / yh_init_state where the call needs them (the context entries take the image size from the
 * state; tracing guides needs the scene), with an asynchronous launch pending, and for rgba_in NULL on a sharded context (yh_set_shard
 * world > 1: gather first and pass the image). YH_E_INVALID: iterations outside 0 .. YH_DENOISE_MAX_ITERATIONS, a NULL params or
 * output, a guide plane the parameters need missing (object always; normal / position where their sigma is > 0; albedo where
 * `demodulate` is set), a device image that is not 16-byte aligned, an unknown form. Every refusal comes before the first write. */
#define YH_DENOISE_MAX_ITERATIONS 6
typedef struct yh_denoise_params {
  int   iterations;
  float sigma_color, sigma_normal, sigma_position;
  int   demodulate, match_object;
} yh_denoise_params;
/* The defaults: 5 iterations, sigma_color 4, sigma_normal 0.5, sigma_position = 0.05 x the diagonal of the uploaded scene's bounds
 * (0 = off with ctx NULL or before an upload), demodulate 1, match_object 1. Settled on the CPU with yh_atrous_filter against the
 * quality condition of tests/test_denoise.py (profiles/denoise/quality.txt).                                                      */
int yh_denoise_default_params(const yh_context* ctx, yh_denoise_params* p);
/* Everything a DEVICE pointer: rgba_in / rgba_out float4 images of the state's size (rgba_in NULL: the context's own render, accum /
 * samples; rgba_out may be rgba_in). guides NULL: the call traces its own centre-mode guides into temporary planes (albedo only
 * when `demodulate` is set); else the struct's object, normal, position, albedo planes as yh_trace_gbuffer_device writes them.    */
int yh_denoise_image_device(yh_context* ctx, const yh_denoise_params* p, const void* rgba_in, const yh_gbuffer* guides, void* rgba_out);
/* The same with HOST pointers, staged as yh_trace_gbuffer stages its planes; the guides are traced by the call. rgba_in may be a
 * gathered multi-GPU image (yh_gather_framebuffer).                                                                               */
int yh_denoise(yh_context* ctx, const yh_denoise_params* p, const float* rgba_in, float* rgba_out);
/* The context's own render, denoised, then the tone map of yh_download_display, as bytes.                                         */
int yh_denoise_display(yh_context* ctx, const yh_denoise_params* p, float exposure, int filmic, int srgb, uint8_t* rgba8);
/* The filter at unit level on the caller's arrays (HOST pointers; w x h pixels; rgba 4, normal / position / albedo 3 floats per
 * pixel, NULL allowed where the parameters do not read them). yh_atrous_filter: the host's form (no GPU, no context), the
 * restatement the device is compared with. yh_atrous_filter_gpu: the same arrays through the device kernels; form 0: every tap
 * from memory; form 1: the levels with s <= 4 from a 16 x 16 tile staged with its halo in LDS. Same bits, all three.              */
int yh_atrous_filter(int w, int h, const yh_denoise_params* p, const float* rgba, const int* object, const float* normal,
    const float* position, const float* albedo, float* out);
int yh_atrous_filter_gpu(yh_context* ctx, int form, int w, int h, const yh_denoise_params* p, const float* rgba, const int* object,
    const float* normal, const float* position, const float* albedo, float* out);
/* Developer diagnostics: the event times in ms of the last yh_atrous_filter_gpu, kernel by kernel — the pack step, then each
 * level. Writes min(capacity, 1 + iterations) numbers, returns 1 + iterations of that call (0: none yet).                         */
int yh_atrous_level_ms(const yh_context* ctx, float* ms, int capacity);

/* TEMPORAL (an extension: the reference has no counterpart; the temporal stage of SVGF, Schied et al. 2017, in front of the filter
 * above). The render of the previous step is reprojected into the new view through the CENTRE-mode position plane, validated against
 * ids and positions, and blended with the new render by sample count.
 * Per pixel p = (i, j) of a W x H image: colour c (float4) with n >= 1 samples in it, id (-1: a miss), world position x. The history:
 * per pixel an accumulated rgb with an integer length (samples in it, 0: none), id and position; the camera it was made under; per
 * object the frame at that time and a flag `usable`. dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z throughout.
 *   1 pass-through     a miss, or a pixel with a channel of c.rgb not finite: out has c's bits, length_out = 0
 *   2 previous point   y = x when the object's previous frame has the bits of its current frame (12 floats) or no motion is given;
 *                      else y = transform_point(prev_frame[id], transform_point(inverse(frame[id], non_rigid), x)) as the object
 *                      rows are made (unit/object_math.h). usable[id] == 0: no history. (An id outside the object list: static.)
 *   3 projection       into the PREVIOUS camera (frame axes ax, ay, az, origin o), the inverse of the centre-mode ray: d = y - o,
 *                      lx = dot(d, ax), ly = dot(d, ay), lz = dot(d, az); no history unless lz < 0;
 *                      u = 0.5 - (lens lx) / (film_x lz), v = 0.5 + (lens ly) / (film_y lz), fx = u W - 0.5, fy = v H - 0.5;
 *                      no history unless both are finite, -1 < fx < W and -1 < fy < H
 *   4 taps             when the previous camera's 17 floats have the current camera's bits and step 2 gave y = x by its bit-equal
 *                      rule: the one tap (i, j) with weight 1 (a still view accumulates without blur). Otherwise i0 = floor(fx),
 *                      tx = fx - i0, j0 = floor(fy), ty = fy - j0, four taps (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1)
 *                      with weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty
 *   5 tap validity     inside the image; length > 0; its id equals the pixel's where `match_object` is set; its rgb finite;
 *                      |y - x_q|^2 <= sigma_position^2 (no test when sigma_position <= 0). A tap of weight 0 is not added.
 *   6 history          one float accumulator per channel and one for the weights, summed in tap order: S = sum w; no history
 *                      unless S > 0; h = sum w c_q / S; N = min(the smallest length among the added taps, max_history)
 *   7 blend            a = (float)n / (float)(N + n); out.rgb = h + (c.rgb - h) a; out.a = c.a (alpha is never blended);
 *                      length_out = N + n. Without a history: out has c's bits and length_out = n.
 *   8 new history      out.rgb with length_out, the current id and position, the current camera and frames
 * + - x / and comparisons only (unit/reproject_math.h, one text for host and device), so device, host and a float32 restatement
 * give the same bits.
 * The context keeps the history (two float4 planes per pixel, twice over; the camera; the objects' frames; `usable`). It SURVIVES
 * yh_update_camera, yh_update_objects (an object whose material changed is unusable until the next accumulate), yh_update_shape /
 * yh_refit_shape and their device forms (the shape's objects are unusable until the next accumulate) and a yh_init_state of the same
 * image size; it is DROPPED by yh_upload_scene, a yh_init_state of another size, yh_update_materials, yh_update_environments, any
 * change of the light list, and yh_temporal_reset: the next accumulate then starts afresh.
 * The entry points change no accumulator, stream, sample count, item cost, trial record or launch shape. Blocking on the context's
 * stream; yh_last_trace_ms reports the kernels' event time and launch count (the feature pass included where the call runs it).
 * YH_E_STATE before yh_upload_scene / yh_init_state, with an asynchronous launch pending, for rgba_in NULL with no sample traced, and
 * for rgba_in NULL on a sharded context (gather first and pass the image). YH_E_INVALID: NULL params, max_history < 1, samples_in < 1
 * with an image given, guides without the object or the position plane, a device image that is not 16-byte aligned. Every refusal
 * comes before the first write.                                                                                                    */
typedef struct yh_temporal_params {
  int   max_history;    /* in samples: the cap of a history's length before the blend */
  float sigma_position; /* world units */
  int   match_object;
} yh_temporal_params;
/* The defaults: max_history 4, sigma_position = 0.2 x the diagonal of the uploaded scene's bounds as they are now (0 = off with ctx
 * NULL or before an upload), match_object 1; settled with yh_reproject on an eight-step orbit (profiles/temporal/quality.txt).       */
int yh_temporal_default_params(const yh_context* ctx, yh_temporal_params* p);
/* Everything a DEVICE pointer: rgba_in a float4 image of the state's size with samples_in samples in it (NULL: the context's own
 * render and its sample count; samples_in is not read); guides NULL: the call traces the centre-mode object and position planes
 * itself, else those two planes of the struct; rgba_out the accumulated image (may be rgba_in; NULL: the history is only updated). */
int yh_temporal_accumulate_device(yh_context* ctx, const yh_temporal_params* p, const void* rgba_in, int samples_in, const yh_gbuffer* guides,
    void* rgba_out);
/* The same with HOST pointers, staged.                                                                                             */
int yh_temporal_accumulate(yh_context* ctx, const yh_temporal_params* p, const float* rgba_in, int samples_in, const yh_gbuffer* guides,
    float* rgba_out);
/* The context's own render accumulated, then yh_denoise's filter on the accumulated image (dp NULL: no filter) — one feature pass
 * serves both stages — then the tone map of yh_download_display, as bytes.                                                         */
int yh_temporal_display(yh_context* ctx, const yh_temporal_params* tp, const yh_denoise_params* dp, float exposure, int filmic, int srgb,
    uint8_t* rgba8);
int yh_temporal_reset(yh_context* ctx);
/* The history's lengths, one int per pixel (lengths may be NULL). Returns the pixel count, 0 without a history, < 0 on an error.   */
int yh_temporal_lengths(yh_context* ctx, int* lengths);
/* One step at unit level on the caller's arrays (HOST pointers; w x h pixels): rgba (4 floats per pixel) with `samples` samples,
 * object, position (3) of the current frame; the history hist_rgba (4 floats per pixel, alpha not read: a previous out_rgba),
 * hist_length, hist_object, hist_position (hist_length NULL: no history at all, the four are not read); both cameras; frames /
 * prev_frames: 12 floats per object, num_objects of them, and usable (NULL: all are) — frames NULL: no motion is given.
 * Writes out_rgba (may be rgba) and out_length; with object and position they are the next step's history.
 * yh_reproject: the host's form (no GPU, no context). yh_reproject_gpu: the same arrays through the device kernel. Same bits.      */
int yh_reproject(int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position,
    const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position, const yh_camera* camera,
    const yh_camera* prev_camera, int num_objects, const float* frames, const float* prev_frames, const int* usable, float* out_rgba,
    int* out_length);
int yh_reproject_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object,
    const float* position, const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position,
    const yh_camera* camera, const yh_camera* prev_camera, int num_objects, const float* frames, const float* prev_frames,
    const int* usable, float* out_rgba, int* out_length);

/* VARIANCE (an extension: the reference has no counterpart; the variance estimate of SVGF, Schied et al. 2017, and the filter it steers).
 * A third image pass beside DENOISE and TEMPORAL: luminance moments ride through TEMPORAL's reprojection (stage M), a spatial estimate
 * stands in where the moment history is short (stage S), and the a-trous levels filter the variance with the colour and scale their
 * colour edge stop by it (stage F). lum(v) = (0.2126f v.x + 0.7152f v.y) + 0.0722f v.z. + - x / and comparisons only
 * (unit/variance_math.h, one text for host and device), so device, host and a float32 restatement give the same bits.
 *   M moments          per pixel, besides TEMPORAL's quantities: an optional albedo plane and a moment history {M1, M2, steps}, steps an
 *                      int, 0: none. l = lum(c.rgb / effective albedo), DENOISE's effective albedo (1 without the plane, 1 on a miss);
 *                      m = (l, l l). Taps, weights, validity, S, N and the blend factor a are TEMPORAL's steps 1 - 7, computed once and
 *                      shared with the colour: the colour output and length_out have yh_reproject's bits whatever the moments do.
 *                      Hm = sum w m_q / S over the added taps, summed in tap order; T = the smallest steps among them. There is a moment
 *                      history when there is a colour history, T > 0 and both of Hm are finite: M_out = Hm + (m - Hm) a and
 *                      steps_out = min(T, YH_VARIANCE_MAX_STEPS - 1) + 1; without one M_out = m and steps_out = 1. A pass-through pixel
 *                      (TEMPORAL step 1) gets M_out = 0 and steps_out = 0. vt = d > 0 ? d : 0 with d = M2_out - M1_out M1_out.
 *   S spatial          after M, over its outputs. steps_out >= min_steps: var = vt. steps_out = 0: var = 0. Otherwise a 7 x 7 window,
 *                      dy = -3..3 outer, dx = -3..3 inner; a tap counts when it lies inside the image, its steps > 0, it has the pixel's id
 *                      where `match_object` is set, |x_p - x_q|^2 <= sigma_position^2 of the temporal parameters (TEMPORAL's dot; no test
 *                      when sigma_position <= 0), and both its moments are finite. Weight 1, one float accumulator per moment, summed
 *                      in tap order, k the count: A = sum M / (float)k, e = A2 - A1 A1, vs = e > 0 ? e : 0 (0 with no tap),
 *                      var = vt > vs ? vt : vs.
 *   F level            per pixel the working colour u of DENOISE and a variance v; the guides are DENOISE's.
 *                      g = sum k3 v_q / sum k3 over the 3 x 3 neighbours at spacing 1 whatever the level, dy outer, dx inner,
 *                      k3 = 1/4, 1/8, 1/16 for |dx| + |dy| = 0, 1, 2; taps outside the image, of another id under `match_object`, or
 *                      with v not finite are skipped; g = 0 with no tap left. The 25 taps are DENOISE's with its h, xn and xx;
 *                      xl = sigma_luminance > 0 ? (lum(u_p) - lum(u_q))^2 / (sigma_luminance^2 g + epsilon) : 0, x = xn + xx + xl,
 *                      w = h / (1 + x + 0.5 x x). A tap is skipped under DENOISE's rules and when v_q is not finite.
 *                      u' = sum w u_q / sum w, v' = sum w w v_q / (sum w sum w). A pixel DENOISE passes unchanged (a miss, sum w = 0,
 *                      u_p not finite) passes u and v unchanged. After the last level the albedo comes back and the input's alpha; the
 *                      variance stays that of the working colour's luminance. With sigma_luminance <= 0 the rgb output has the bits of
 *                      yh_atrous_filter with sigma_color = 0 and otherwise the same parameters.
 * The moment history lives and dies with TEMPORAL's colour history: kept and dropped by the same events, under the same `usable` rule. A
 * plain yh_temporal_accumulate* in between advances the colour and marks the moment history as none: the next variance call starts at
 * steps = 1 with the spatial estimate. The entries change no accumulator, stream, sample count, item cost, trial record or launch shape.
 * Refusals are TEMPORAL's and DENOISE's, and YH_E_INVALID for guides without the albedo plane where `demodulate` is set, min_steps < 1
 * and an epsilon that is not > 0; every refusal comes before the first write.                                                          */
#define YH_VARIANCE_MAX_STEPS 1024
typedef struct yh_variance_params {
  int   iterations;
  float sigma_luminance, sigma_normal, sigma_position;
  int   demodulate, match_object;
  float epsilon;
  int   min_steps;
} yh_variance_params;
/* The defaults: 4 iterations, sigma_luminance 2, epsilon 1e-2, min_steps 4, settled on the CPU with the host's forms on the eight-step
 * orbit of tools/variance_quality.py (profiles/variance/quality.txt); sigma_normal, sigma_position (0.05 x the scene's diagonal, 0
 * with ctx NULL or before an upload), demodulate and match_object are those of yh_denoise_default_params.                             */
int yh_variance_default_params(const yh_context* ctx, yh_variance_params* p);
/* Stages M and S on the context's history. Everything a DEVICE pointer, as yh_temporal_accumulate_device takes them; guides NULL: the
 * call traces object, position and (where vp->demodulate is set) albedo itself. variance_out: one float per pixel (NULL: kept in the
 * context only, for yh_denoise_variance_image_device).                                                                               */
int yh_temporal_accumulate_variance_device(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, const void* rgba_in,
    int samples_in, const yh_gbuffer* guides, void* rgba_out, float* variance_out);
/* The same with HOST pointers, staged.                                                                                             */
int yh_temporal_accumulate_variance(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, const float* rgba_in,
    int samples_in, const yh_gbuffer* guides, float* rgba_out, float* variance_out);
/* Stage F. DEVICE pointers as yh_denoise_image_device takes them (rgba_in is required); variance_in NULL: the variance the context
 * kept from its last yh_temporal_accumulate_variance* (YH_E_STATE without one of the state's size); variance_out may be NULL.        */
int yh_denoise_variance_image_device(yh_context* ctx, const yh_variance_params* vp, const void* rgba_in, const float* variance_in,
    const yh_gbuffer* guides, void* rgba_out, float* variance_out);
/* The same with HOST pointers, staged; the guides are traced by the call where `guides` is NULL.                                    */
int yh_denoise_variance_image(yh_context* ctx, const yh_variance_params* vp, const float* rgba_in, const float* variance_in,
    const yh_gbuffer* guides, float* rgba_out, float* variance_out);
/* One feature pass (object, normal, position, albedo), then M, S and F on the context's own render, then the tone map, as bytes.     */
int yh_svgf_display(yh_context* ctx, const yh_temporal_params* tp, const yh_variance_params* vp, float exposure, int filmic, int srgb,
    uint8_t* rgba8);
/* The moment history's steps, one int per pixel (steps may be NULL), as yh_temporal_lengths: the pixel count, 0 without a moment
 * history, < 0 on an error.                                                                                                         */
int yh_temporal_steps(yh_context* ctx, int* steps);
/* The stages at unit level on the caller's arrays (HOST pointers; w x h pixels). The plain names are the host's forms (no GPU, no
 * context), the _gpu names the same arrays through the device kernels. Same bits.
 * yh_reproject_moments: yh_reproject's arguments, plus albedo (3 floats per pixel, NULL: none), hist_moments (2 floats per pixel) and
 * hist_steps of the previous step (read only where hist_length is given; both NULL: no moment history, steps 0 everywhere), and the
 * outputs out_moments and out_steps.
 * yh_variance_spatial: stage S over a step's outputs; tp gives sigma_position and match_object.
 * yh_atrous_variance_filter: stage F, all levels; variance one float per pixel; out may be rgba, out_variance may be variance or NULL.
 * form 0: every tap from memory; form 1: the levels with s <= 4 from a 16 x 16 tile staged with its halo in LDS. After
 * yh_atrous_variance_filter_gpu, yh_atrous_level_ms reports its kernels as it does yh_atrous_filter_gpu's.                         */
int yh_reproject_moments(int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object, const float* position,
    const float* albedo, const float* hist_rgba, const int* hist_length, const int* hist_object, const float* hist_position,
    const float* hist_moments, const int* hist_steps, const yh_camera* camera, const yh_camera* prev_camera, int num_objects,
    const float* frames, const float* prev_frames, const int* usable, float* out_rgba, int* out_length, float* out_moments, int* out_steps);
int yh_reproject_moments_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* p, const float* rgba, int samples, const int* object,
    const float* position, const float* albedo, const float* hist_rgba, const int* hist_length, const int* hist_object,
    const float* hist_position, const float* hist_moments, const int* hist_steps, const yh_camera* camera, const yh_camera* prev_camera,
    int num_objects, const float* frames, const float* prev_frames, const int* usable, float* out_rgba, int* out_length, float* out_moments,
    int* out_steps);
int yh_variance_spatial(int w, int h, const yh_temporal_params* tp, int min_steps, const float* moments, const int* steps, const int* object,
    const float* position, float* out_variance);
int yh_variance_spatial_gpu(yh_context* ctx, int w, int h, const yh_temporal_params* tp, int min_steps, const float* moments, const int* steps,
    const int* object, const float* position, float* out_variance);
int yh_atrous_variance_filter(int w, int h, const yh_variance_params* p, const float* rgba, const float* variance, const int* object,
    const float* normal, const float* position, const float* albedo, float* out, float* out_variance);
int yh_atrous_variance_filter_gpu(yh_context* ctx, int form, int w, int h, const yh_variance_params* p, const float* rgba, const float* variance,
    const int* object, const float* normal, const float* position, const float* albedo, float* out, float* out_variance);

/* Work counters of the launches since the last reset (instrumented build of
 * the same kernel; 0 = ok).                                                  */
int yh_trace_samples_counted(yh_context* ctx, int nsamples, yh_workcounts* out);

/* HIP-event time in milliseconds of the most recent yh_trace_samples launch
 * sequence on the context's own stream, and the number of kernel launches.   */
int yh_last_trace_ms(const yh_context* ctx, float* ms, int* launches);

/* Which sample-loop kernel the most recent yh_trace_samples launch ran (the host picks per launch from
 * measured times; every choice renders the same bits): 0 = k_trace, a quad of lanes per path, 512 threads
 * x 4 waves per SIMD; 1 = the same at 256 x 5 (dense images); 3 = k_stream, one lane per path (dense
 * images); 4 = k_trace with an OCTET per path over 8-wide BVH nodes, 7 = the same with leaf pairs, 6 =
 * SIXTEEN lanes per path over 16-wide nodes, 8 = the same with leaf groups (launches bound by the chain of
 * one path: few expensive pixels per GPU); 5 = side by side in one launch: the few items that top every
 * launch of a sparse image as octets, everything else as quads; 2 = quads over 8-wide nodes: a developer
 * build, never chosen (YHAIR_SHAPE=n forces a shape; YHAIR_DEVICE_SHARE=k tells the choice that k processes render on
 * this device at once). < 0 = nothing launched yet (or an error code). With
 * yh_trace_params::hair_exact it is always 0.                                                            */
int yh_launch_shape(const yh_context* ctx);
/* The measurements behind that choice on the current image: for launch shape k < count, the milliseconds per sample
 * of its fastest 32-sample trial launch (0 = not tried, < 0 = cannot run on this device) and the number of trials.
 * Returns the number of launch shapes (9), or a negative error code.                                               */
int yh_kernel_trials(const yh_context* ctx, double* ms_per_sample, int* trials, int count);
/* 1 while a candidate kernel of the current image still wants a timing trial — the next yh_trace_samples of 64 samples or
 * more will start with a 32-sample launch of it — else 0: a caller that times its launches (bench.py) keeps warming up
 * until this is 0. The record of an image is kept per process and, when the caller opted in (yh_set_trial_cache_dir), on disk.
 * Replaces nothing in the reference (host/launch_plan.cpp: pick_launch_shape).                                          */
int yh_trials_pending(const yh_context* ctx);
/* The kernel-trial record ON DISK (process-wide, opt-in: a library call writes no file unless asked to). `dir` = a directory
 * (created when needed) that holds trials_v2.txt, one appended line per image, keyed by device, the loaded library's
 * fingerprint, scene, image size, shard and bounces: an image found there runs no trial at all, so two processes (two
 * ranks, two runs) render one image with one kernel. NULL or "" = no file (the default). yscenetrace / ysceneitraces /
 * bench.py pass yh_default_trial_cache_dir() = $XDG_CACHE_HOME/yhair or ~/.cache/yhair. The environment's YHAIR_CACHE_DIR
 * names a directory too (and wins); YHAIR_NO_DISK_CACHE switches the file off whatever was set. No reference counterpart. */
int         yh_set_trial_cache_dir(const char* dir);
const char* yh_default_trial_cache_dir(void);

/* Load-balance telemetry: for every tile id (row-major over ceil(W/8) x
 * ceil(H/8) tiles) the time its wavefront spent on it in the most recent
 * launch (0 for tiles of other shards). The UNIT depends on the kernel that
 * ran (yh_launch_shape): k_trace (0, 1) reports ticks of the 100 MHz device
 * wall clock, k_stream (3) the BVH steps of the tile's rays — both are
 * relative costs for scheduling, comparable within one launch only.
 * `count` = number of tiles the caller's buffer holds.                       */
int yh_tile_costs(yh_context* ctx, uint32_t* ticks, int count);
/* The same per WORK ITEM (a tile's four 4x4-pixel quadrants, item = 4 * tile + quadrant: what a wavefront takes
 * at a time and what the launch's hand-out order is planned from). `count` >= 4 * number of tiles.              */
int yh_item_costs(yh_context* ctx, uint32_t* costs, int count);

/* ------------------------------------------------------------------------ */
/* Unit-level API: replaces yocto::extension and the intersect_* functions    */
/* (batched, host arrays in / host arrays out; device does the arithmetic)    */
/* ------------------------------------------------------------------------ */

/* hair_brdf as 30 floats: sigma_a[3] alpha eta h v[4] s sin_2k_alpha[3]
 * cos_2k_alpha[3] gamma_o world_to_brdf[12]  (yocto_extension.h:97-113)      */
#define YH_HAIR_BRDF_FLOATS 30

/* The surface lobes of yocto_math.h:1513-1620 (implementation 4307-4755).    */
enum {
  YH_LOBE_DIFFUSE            = 0, /* eval/sample/_pdf  diffuse_reflection         */
  YH_LOBE_SPECULAR           = 1, /* microfacet_reflection(ior, ...)              */
  YH_LOBE_METAL              = 2, /* microfacet_reflection(eta, etak, ...)        */
  YH_LOBE_TRANSMISSION       = 3, /* microfacet_transmission                      */
  YH_LOBE_REFRACTION         = 4, /* microfacet_refraction                        */
  YH_LOBE_DELTA_SPECULAR     = 5, /* delta_reflection(ior, ...)                   */
  YH_LOBE_DELTA_METAL        = 6, /* delta_reflection(eta, etak, ...)             */
  YH_LOBE_DELTA_TRANSMISSION = 7, /* delta_transmission                           */
  YH_LOBE_DELTA_REFRACTION   = 8, /* delta_refraction                             */
  YH_LOBE_COUNT              = 9
};
/* yh_surface_bsdf_batch output per item: diffuse[3] specular[3] metal[3]
 * transmission[3] refraction[3] roughness opacity, the five lobe pdfs, then
 * f*|cos| [3], pdf and the sampled incoming [3] (delta forms when roughness
 * is 0, pt.cpp:495).                                                        */
#define YH_SURFACE_BSDF_FLOATS 29

/* eval_hair_brdf (yocto_extension.cpp:127-177). materials: n x yh_material
 * (only hair fields read); v: n; normal, tangent: 3n; out: 30n.              */
int yh_hair_brdf_batch(yh_context* ctx, int n, const yh_material* materials,
    const float* v, const float* normal, const float* tangent, float* brdf);
/* eval_hair_scattering (yocto_extension.cpp:255-336): out 3n.                */
int yh_hair_eval_batch(yh_context* ctx, int n, const float* brdf,
    const float* outgoing, const float* incoming, float* f);
/* sample_hair_scattering (yocto_extension.cpp:399-479): rn 2n -> incoming 3n */
int yh_hair_sample_batch(yh_context* ctx, int n, const float* brdf,
    const float* outgoing, const float* rn, float* incoming);
/* sample_hair_scattering_pdf (yocto_extension.cpp:481-551): out n.           */
int yh_hair_pdf_batch(yh_context* ctx, int n, const float* brdf,
    const float* outgoing, const float* incoming, float* pdf);
/* README.md:20 / BASELINE.json call it eval_hair_scattering_pdf: same entry. */
int yh_hair_eval_pdf_batch(yh_context* ctx, int n, const float* brdf,
    const float* outgoing, const float* incoming, float* pdf);

/* The hair path of a shaded hit, row by row: what the sample-loop kernels run at
 * a hair hit (csrc/dev_path.h) — hair_setup, hair_prepare, hair_sample from
 * that hair_out, then the fused eval + pdf, at `incoming` and at the sampled
 * direction — on the material row that yh_upload_scene makes of `materials`
 * (the per-lobe constants computed on the host, not on the device as the
 * yh_hair_*_batch calls above derive them). form 0: a quad per row, as the
 * quad kernels run it (the lobe pdfs come from lanes 2-3 of the quad, gamma_t
 * from lane 0, lobe p is evaluated on lane p); form 1: a lane per row, as the
 * streaming kernel runs it. exact 0: the default arithmetic of the BSDF;
 * exact 1: the exact arithmetic (yh_trace_params::hair_exact), form 0 only —
 * form 1 with exact 1 is YH_E_INVALID, as are a form or exact other than 0 / 1.
 * materials: n x yh_material (only hair fields read); v: n; normal, tangent,
 * outgoing, incoming: 3n; rn: 2n. out: YH_HAIR_SHADE_FLOATS per row = f[3] and
 * pdf at `incoming`, the sampled direction[3], f[3] and pdf at it, the four
 * lobe pdfs.                                                                 */
#define YH_HAIR_SHADE_FLOATS 15
int yh_hair_shade_batch(yh_context* ctx, int form, int exact, int n,
    const yh_material* materials, const float* v, const float* normal,
    const float* tangent, const float* outgoing, const float* incoming,
    const float* rn, float* out);

/* The pbrt `curve` -> hair-line conversion of the reference's pbrt loader
 * (libs/yocto/yocto_pbrt.h:1751-1797): each curve's first four control points
 * become a strand of five vertices (Bezier at u = 0, 1/4, 1/2, 3/4, 1), with
 * tangents as "normals" and radius = lerp(width0, width1, u), joined by four
 * lines. P: 12n; width0, width1: n; out: positions 15n, normals 15n, radius
 * 5n, lines 8n ints (vertex indices start at base_vertex + 5 * curve).       */
int yh_curves_to_lines(yh_context* ctx, int n, const float* P, const float* width0,
    const float* width1, int base_vertex, float* positions, float* normals,
    float* radius, int* lines);

/* build_bvh (yocto_pathtrace.cpp:598-650) on the host, exactly as
 * yh_upload_scene builds it: boxes = n x (min[3], max[3]). Call with nodes =
 * NULL to get the node count; nodes = 8 floats per node (bbox min, bbox max,
 * then as int bits: start, num | internal << 16 | axis << 24), primitives = n
 * ints (leaf order). Needs no GPU and no context. Returns the node count.     */
int yh_bvh_build(int n, const float* boxes, float* nodes, int* primitives);
/* The same tree as the device traverses it: `width` (4, 8 or 16) children per node = two, three or four levels of
 * the binary tree collapsed into one record of `width` 32-byte slots {min.xyz, max.x} {max.yz, ref, axes}
 * (yocto-hair_amd/host/bvh_build.h). ref: 0xFFFFFFFF empty; top two bits set = leaf (count << 27 | first
 * primitive position); else the index of the child node. axes: the split axes of the collapsed binary nodes, from
 * which a traversal ranks the children into the reference's near-first order (yocto_pathtrace.cpp:887-893).
 * Writes width * 8 floats per node to `slots` (NULL: count only); returns the number of nodes. No GPU needed.       */
int yh_bvh_build_wide(int n, const float* boxes, int width, float* slots);

/* The same tree built on the GPU (csrc/bvh_gpu.hip; what yh_upload_scene uses for
 * shapes of 32 768 primitives and more). Same arguments and result as yh_bvh_build;
 * the two are compared node for node in the tests.                            */
int yh_bvh_build_gpu(yh_context* ctx, int n, const float* boxes, float* nodes, int* primitives);
/* ... and its wide collapse made on the GPU too (csrc/bvh_gpu.hip: what yh_upload_scene runs for EVERY shape since round 6 — the host's
 * collapse_wide* of yh_bvh_build_wide are the restatement it is tested against). Same arguments and result as yh_bvh_build_wide, in the form the
 * traversal kernels read: a child's ref is the index of its FIRST SLOT (width x the child node's index), and for width 4 bits 8-11 of `axes`
 * hold the occupied slots.                                                                                                              */
int yh_bvh_build_wide_gpu(yh_context* ctx, int n, const float* boxes, int width, float* slots);
/* REFIT of such a tree (what yh_refit_shape runs per width): `slots`, in and out, holds a `width`-wide tree over n primitives in the
 * form of yh_bvh_build_wide_gpu; `boxes` are the primitives' NEW boxes, in primitive order; `primitives` is the leaf order of
 * yh_bvh_build / yh_bvh_build_gpu. Every occupied slot's box is formed again bottom-up; ref and axes are not written. Returns the
 * node count. `slots` MUST hold every node its references name: the count is not an argument, so the call finds the nodes by walking
 * the references from node 0, level by level, and checks as it goes — an internal reference must name the next node in breadth-first
 * order (width x its index) and no node past the n-th, a leaf must lie inside the n primitives, `primitives` must be indices below
 * n — before any box is read or written; what fails a check is YH_E_INVALID and leaves `slots` as it was. It cannot tell a buffer that
 * is shorter than the tree it describes. yh_bvh_refit_wide is the host restatement (no GPU, no context) that yh_bvh_refit_wide_gpu —
 * the kernel of yh_refit_shape, one launch per level — is compared with.                                                              */
int yh_bvh_refit_wide(int n, const float* boxes, const int* primitives, int width, float* slots);
int yh_bvh_refit_wide_gpu(yh_context* ctx, int n, const float* boxes, const int* primitives, int width, float* slots);

/* One surface lobe (kind = YH_LOBE_*) of yocto_math.h:1513-1620 (implementation
 * 4427-4755): eval_* (value times |cos|), sample_*_pdf and sample_* in one
 * call. params: 8n (ior, roughness [= brdf.roughness, already squared], eta[3],
 * etak[3]); normal, outgoing, incoming: 3n; rn: 3n (rnl, rn.x, rn.y);
 * out: 7n (f[3], pdf, sampled incoming[3]).                                   */
int yh_surface_lobe_batch(yh_context* ctx, int kind, int n, const float* params,
    const float* normal, const float* outgoing, const float* incoming,
    const float* rn, float* out);
/* The lobe mixture of a non-hair material: eval_brdf (yocto_pathtrace.cpp:
 * 405-471) followed by eval_brdfcos / sample_brdfcos / sample_brdfcos_pdf or,
 * for a delta mixture, eval_delta / sample_delta / sample_delta_pdf
 * (:1069-1280). out: YH_SURFACE_BSDF_FLOATS per item.                          */
int yh_surface_bsdf_batch(yh_context* ctx, int n, const yh_material* materials,
    const float* normal, const float* outgoing, const float* incoming,
    const float* rn, float* out);
/* intersect_scene_bvh (yocto_pathtrace.cpp:934-1046) on the uploaded scene.
 * rays: 8n floats (o[3] d[3] tmin tmax). Outputs per ray: object, element
 * (-1 on miss), uv[2], distance.                                             */
int yh_intersect_batch(yh_context* ctx, int n, const float* rays, int* object,
    int* element, float* uv, float* distance);
/* intersect_scene_bvh (yocto_pathtrace.cpp:934-1046) through the traversal of
 * the PLAIN 512-thread sample-loop kernels, with the scene-level table staged
 * in LDS as a launch stages it and in the form a launch on this scene takes
 * (the scene level resolved once per ray where it is one leaf node). form 0:
 * a quad per ray over 4-wide nodes (launch shape 0, the quad half of shape
 * 5); form 1: an octet per ray over 8-wide nodes (the octet half of shape 5).
 * Forms 2-6 run the traversal of the 256-thread launch shapes, with their
 * workgroup size and LDS stack stride, in the form without the once-per-ray
 * scene level (none of those shapes has one):
 *   2  a quad per ray, the dense form              (launch shape 1)
 *   3  an octet per ray over 8-wide nodes          (launch shape 4)
 *   4  an octet per ray with leaf pairs            (launch shape 7)
 *   5  sixteen lanes per ray over 16-wide nodes    (launch shape 6)
 *   6  sixteen lanes per ray with leaf groups      (launch shape 8)
 * form | YH_INTERSECT_TABLE_IN_MEMORY (forms 3-6 only): the scene level read
 * from memory, as the GENERAL variants of those shapes read a table that does
 * not fit LDS — a 4-wide scene node then runs in every quad of the octet or
 * the sixteen. Arguments and results as yh_intersect_batch. YH_E_INVALID for
 * an unknown form, and — the memory-table forms apart — for a scene that
 * renders with the GENERAL kernel variants.                                  */
#define YH_INTERSECT_FORMS 7
#define YH_INTERSECT_TABLE_IN_MEMORY 16
int yh_intersect_plain_batch(yh_context* ctx, int form, int n, const float* rays,
    int* object, int* element, float* uv, float* distance);
/* The lanes that own a ray in `form` of yh_intersect_plain_batch (4, 8 or 16);
 * YH_E_INVALID for a form it does not have: the answer the batch gives too.    */
int yh_intersect_plain_form(int form);
/* Whether the plain 512-thread kernels resolve the uploaded scene's scene
 * level once per ray, ahead of the traversal loop (a scene level of ONE leaf
 * node: at most four objects): the number of objects, else 0; YH_E_STATE
 * before yh_upload_scene.                                                    */
int yh_scene_once(const yh_context* ctx);
/* 1 when the uploaded scene is plain, none of its environments has a texture
 * and every light is an environment: light sampling, the light pdf and the
 * environment lookup of the plain 512-thread kernels (launch shapes 0 and 5)
 * then take the counts and the emissions from the kernel argument and fetch
 * nothing; else 0. Follows every edit, as yh_scene_once. YH_E_STATE before
 * yh_upload_scene.                                                          */
int yh_lights_const_env(const yh_context* ctx);
/* Developer diagnostics: the shading pass of the last yh_trace_samples_counted
 * by REGION of a wave iteration, three numbers per region — the waves' cycles
 * in it, the trips that ran it, the lanes it ran with — in the order loop head
 * (path regeneration; outside cyc_shade), miss, fetch (rows, record, normals),
 * hair set-up, sampling branch, BSDF value and pdf, lights pdf, weight and
 * continuation, path end. Writes min(capacity, 27) numbers, returns 27.     */
int yh_shade_regions(const yh_context* ctx, uint64_t* out, int capacity);
/* Developer diagnostics: which work items the next yh_trace_samples_counted
 * launches count — the first `items` of the cost-ordered work list (the most
 * expensive ones by the costs of the launch before; tools/top_items.py:
 * expensive_count says how many are within 5 x of the top), so that the
 * per-iteration figures describe the sample chains a chain-bound launch waits
 * for and not the average over its background items. Every item still runs
 * the instrumented kernel; the others add nothing to the work counts, the
 * cycle stamps, the branch counts and the regions. 0 (the default): every
 * item, as before. Product launches are unaffected.                          */
int yh_set_count_bound(yh_context* ctx, int items);

/* The light code on the uploaded scene, row by row: sample_lights and
 * sample_lights_pdf (yocto_pathtrace.cpp:1283-1358) and eval_environment
 * (:536-547), the very functions the sample-loop kernels call, with their
 * tables staged as a launch stages them. form 0: a quad per row as in the
 * quad kernels (the scene's plain or general variant, as a launch picks it);
 * form 1: a lane per row as in the streaming kernel. position, direction: 3n;
 * rn: 4n (rl, rel, ruv.x, ruv.y); out: 8n = sampled direction[3],
 * sample_lights_pdf at it, sample_lights_pdf at `direction`,
 * eval_environment(direction)[3].                                            */
int yh_lights_batch(yh_context* ctx, int form, int n, const float* position,
    const float* direction, const float* rn, float* out);

/* The homogeneous medium of a path, row by row: what the sample-loop kernels
 * run when a path crosses into a closed transmissive object and flies through
 * it (csrc/dev_path.h: medium_crossing, the free-flight block of path_step;
 * csrc/dev_surface.h: eval_transmittance ... sample_scattering_pdf), on the
 * material row that yh_upload_scene makes of `materials`. Per row:
 *   1. medium_crossing from outside with `normal`, `outgoing`, `incoming`.
 *      tex 0: the row's host-made density. tex 1: the row with its colour
 *      texture set, so that the device derives the density from the row's
 *      colour x texval[0..2] and its transmission x texval[3].
 *   2. the free flight for rl, rd and max_distance: distance, the weight
 *      factor eval_transmittance / sample_transmittance_pdf and that pdf;
 *   3. the scatter for rx, ry: the sampled direction, eval_scattering and
 *      sample_scattering_pdf at `incoming` and at the sampled direction.
 * A row that enters no medium runs 2 and 3 on a zero medium. form 0: a quad
 * per row, as the quad kernels run it; form 1: a lane per row, as the
 * streaming kernel runs it (the medium read back from the path's slot).
 * YH_E_INVALID for n < 1, a NULL pointer, a form or tex other than 0 / 1.
 * normal, outgoing, incoming: 3n; texval: 4n; rn: 5n (rl, rd, max_distance,
 * rx, ry). out: YH_VOLUME_FLOATS per row = in_medium (0 / 1), density[3],
 * scatter[3], anisotropy, distance, weight factor[3], distance pdf, sampled
 * direction[3], f[3] and pdf at `incoming`, f[3] and pdf at the sampled
 * direction.                                                                 */
#define YH_VOLUME_FLOATS 24
int yh_volume_batch(yh_context* ctx, int form, int tex, int n,
    const yh_material* materials, const float* normal, const float* outgoing,
    const float* incoming, const float* texval, const float* rn, float* out);
/* The shading point of a hit, row by row on the uploaded scene with its maps:
 * what the sample loops make of a closest hit before the lobes are sampled
 * (csrc/dev_path.h: eval_hit, eval_hit_fetch_first, eval_texcoord, eval_maps,
 * eval_normalmap, eval_hit_maps, the shading-normal rule and the head of
 * path_step / shade_step up to surface_brdf; csrc/dev_surface.h:
 * eval_texture), the loops' own functions in the order the head of path_step
 * calls them, then medium_crossing from outside with incoming = -outgoing.
 * Per row: object, element (the caller's element; a small kernel inverts the
 * leaf order of the shapes the batch names to find the hit's leaf slot — a
 * diagnostic, like yh_shape_nodes), uv[2], outgoing[3] (as given: not
 * normalised). Each form reads its rows where the loop it stands for reads
 * them:
 *   form 0  launch shape 0 on this scene, a quad per row. Plain scene: object
 *           and material rows from LDS, eval_hit_fetch_first, no maps, no
 *           mixture. General scene: rows from memory, eval_hit +
 *           eval_hit_maps, the mixture unless the material is plain.
 *   form 1  the streaming kernel, a lane per row: rows from LDS on a plain
 *           scene, else from memory; eval_hit (+ eval_hit_maps).
 *   form 2  the 256-thread shape and shade_step, a quad per row: rows from
 *           memory whatever the scene, eval_hit + eval_hit_maps, the mixture
 *           for every material.
 * out: YH_POINT_FLOATS per row, the columns below. Where the loop computes no
 * mixture (a plain material on a plain variant) the row reports what its
 * diffuse-only path works with — the colour as the diffuse weight, roughness
 * and opacity 1, the pdfs (the row's diffuse_pdf, 0, 0, 0, 0) — which is what
 * eval_brdf makes of such a material. The texcoord is the one the loop has:
 * eval_texcoord where the material has a texture or a map, else the element
 * uv it keeps. YH_E_STATE before an upload; YH_E_INVALID for n < 1, a NULL
 * pointer, an unknown form, an object outside the scene or an element outside
 * its shape (found before anything follows the index).                       */
#define YH_POINT_POSITION        0 /* [3] eval_position                                        */
#define YH_POINT_NORMAL          3 /* [3] eval_normal                                          */
#define YH_POINT_SHADING_NORMAL  6 /* [3] eval_shading_normal, the normal map included         */
#define YH_POINT_TEXCOORD        9 /* [2] eval_texcoord                                        */
#define YH_POINT_COLOR_TEX      11 /* [3] eval_texture(color_tex)                              */
#define YH_POINT_EMISSION_TEX   14 /* [3] eval_texture(emission_tex)                           */
#define YH_POINT_EMISSION_TEX_X 17 /*     eval_texture(emission_tex, linear).x                 */
#define YH_POINT_SCATTERING_TEX 18 /* [3] eval_texture(scattering_tex)                         */
#define YH_POINT_EMISSION       21 /* [3] eval_emission                                        */
#define YH_POINT_BSDF           24 /* [22] the leading floats of YH_SURFACE_BSDF_FLOATS: the
                                      five lobe weights, roughness, opacity, the five pdfs     */
#define YH_POINT_DENSITY        46 /* [3] eval_vsdf of the medium entered straight through the */
#define YH_POINT_SCATTER        49 /* [3] surface (pt.cpp:1458-1467 with incoming = -outgoing) */
#define YH_POINT_ANISOTROPY     52 /*     for a material with a volume; zero otherwise         */
#define YH_POINT_FLOATS         53
int yh_point_batch(yh_context* ctx, int form, int n, const int* object,
    const int* element, const float* uv, const float* outgoing, float* out);
/* The quad forms of the trimmed 512-thread kernels next to the plain forms
 * whose bits they render (csrc/dev_surface.h: sample_hemisphere_cos_quad,
 * csrc/dev_math.h: quad_div), a quad per row. normal, a: 3n; rn: 2n (rx, ry);
 * b: n. out: YH_QUAD_FORMS_FLOATS per row = sample_hemisphere_cos_quad[3],
 * sample_hemisphere_cos[3], quad_div(a, b)[3], a / b [3]. YH_E_INVALID for
 * n < 1 or a NULL pointer.                                                   */
#define YH_QUAD_FORMS_FLOATS 12
int yh_quad_forms_batch(yh_context* ctx, int n, const float* normal,
    const float* rn, const float* a, const float* b, float* out);
/* The start and the end of a path, row by row: what every sample of every
 * sample-loop kernel runs around its bounces (csrc/dev_path.h: path_begin
 * with sample_camera / sample_camera_lane, pt.cpp:211-229 and 1676-1682;
 * path_continue, pt.cpp:1499-1507; path_end, pt.cpp:1683-1689). form 0: a
 * quad per row, as the quad loops run them; form 1: a lane per row, as the
 * streaming kernel runs them. Per row of `op`:
 *   YH_PATH_BEGIN     fin: the camera as the kernels hold it, 17 floats =
 *     frame[12], lens, film x, film y, focus, aperture; iin: i, j, w, h; rng:
 *     state, inc. Form 0 runs path_begin; form 1 the four draws (lens u, v,
 *     then pixel u, v) and sample_camera_lane. fout: ray origin[3],
 *     direction[3], then radiance[3] and weight[3]; iout: bounce, hit,
 *     in_medium as path_begin leaves them (form 1: zeros, it runs no
 *     path_begin); state: the stream's state afterwards.
 *   YH_PATH_CONTINUE  fin: weight[3]; iin: bounce, bounces; rng: state, inc.
 *     path_continue: the weight check, Russian roulette from the fifth
 *     bounce on, the bounce count. fout: weight[3]; iout: the flag it
 *     returns (1: the path goes on), bounce; state.
 *   YH_PATH_END       fin: radiance[3], clamp, acc[4]; iin: hit. path_end: a
 *     non-finite radiance becomes zero, one whose largest component exceeds
 *     clamp is scaled by clamp / that component, then acc += {rgb, hit}.
 *     fout: acc[4]. rng, iout and state are not used and may be NULL.
 * YH_E_INVALID for n < 1, an unknown op or form, or a NULL pointer among those
 * the op uses.                                                              */
#define YH_PATH_BEGIN 0
#define YH_PATH_CONTINUE 1
#define YH_PATH_END 2
#define YH_PATH_OPS 3
#define YH_PATH_BEGIN_IN 17
#define YH_PATH_BEGIN_OUT 12
#define YH_PATH_CONTINUE_IN 3
#define YH_PATH_CONTINUE_OUT 3
#define YH_PATH_END_IN 8
#define YH_PATH_END_OUT 4
int yh_path_ends_batch(yh_context* ctx, int op, int form, int n,
    const float* fin, const int* iin, const uint64_t* rng, float* fout,
    int* iout, uint64_t* state);

/* The four Monte-Carlo self-tests of yocto_extension.cpp:555-693 on the
 * device: 0 white_furnace, 1 white_furnace_sampled, 2 sampling_weights,
 * 3 sampling_consistency. Same seeds, counts and thresholds. `worst` (may be
 * NULL) receives the statistic furthest from its target. Returns YH_OK or
 * YH_E_SELFTEST ("TEST FAILED!").                                            */
int yh_selftest(yh_context* ctx, int which, float* worst);

/* ------------------------------------------------------------------------ */
/* Host-side scene I/O (C++ host code, no device work): the minimal JSON +    */
/* PLY + Radiance-HDR reader for the hair scenes, with the reference loader's */
/* semantics (yocto_sceneio.cpp:1064-1418: alphabetical objects, lookat,      */
/* add_radius 0.001, quads_to_triangles).                                     */
/* INSTANCES: an object's "instance": "<name>" names instances/<name>.ply (element `instance`, the twelve float or double properties xx xy xz yx
 * yy yz zx zy zz ox oy oz looked up by name; yocto_sceneio.cpp:848-867,1198-1217). The loaded description holds them EXPANDED, as the
 * reference's command line expands them (apps/yscenetrace/yscenetrace.cpp:150-181): in the object's alphabetical place one yh_object per
 * frame, in file order, frame = instance_frame * object_frame (yocto_math.h:2871-2873, the same float operations), all with the object's
 * shape and material; a file without frames makes the object vanish, "" is no instance, a file named by several objects is read once. Each
 * copy of an emissive object is a light of its own. A missing file, element or property is an error that names the file. "subdiv"
 * (subdivision surfaces) is refused.                                                                                                    */
/* ------------------------------------------------------------------------ */
typedef struct yh_scene_file yh_scene_file;
yh_scene_file*       yh_scene_load(const char* json_path, const char* camera,
          char* error, int error_len);
const yh_scene_desc* yh_scene_get(const yh_scene_file* scene);
/* The materials' maps of a loaded scene (the *_tex keys of sceneio.cpp:1298-1317): num_materials entries, for
 * yh_upload_scene_maps. translucency_tex and displacement_tex are loaded (a missing file is an error) and used by
 * nothing; coat_tex and spectint_tex, which the reference's loader does not read, are ignored.                      */
const yh_material_maps* yh_scene_get_maps(const yh_scene_file* scene);
void                 yh_scene_free(yh_scene_file* scene);
/* save_image for .pfm (3 channels, top row first as the reference writes it,
 * yocto_image.cpp:1527-1556) and .hdr.                                       */
int yh_save_image(const char* path, int width, int height, const float* rgba,
    char* error, int error_len);

#ifdef __cplusplus
}
#endif
#endif /* YHAIR_H_ */
