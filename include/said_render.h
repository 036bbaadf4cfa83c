/*
 * said_render.h — C ABI of the blendshape-animation renderer (said_amd/csrc/render.hip, renderer.cpp), in libsaid_hip.so beside said_hip.h.
 *
 * The reference (script/rendering/render_visual.py, driven by script/render.py and script/test_render.py) turns a (T, K) coefficient sequence
 * into T images of 800 x 800 through trimesh and pyrender / OpenGL.  Here the same sequence is rendered by five kernels per chunk of frames:
 * vertices v_t = n + B_delta w_t (and, against a target sequence, the colour-mapped per-vertex difference), angle-weighted vertex normals
 * (a face pass and a gather), a per-triangle set-up (rotation, pinhole projection) and a tile rasteriser that shades the surviving fragment
 * in place.  DESIGN.md section 15
 * is the specification: projection, coverage, depth test, interpolation and the shading formula, symbol by symbol.
 *
 * Conventions are those of said_metrics.h: 0 on success, said_render_last_error(ctx) (NULL for create failures) gives the message; `*_dev` are
 * device pointers, `*_host` host memory; `stream` is a hipStream_t.  Nothing aborts.  All arithmetic is fp32, there are no atomics and every
 * sum runs in a fixed order: a frame's pixels do not depend on the chunk it is rendered in, and equal inputs give bit-identical outputs.
 * said_render_set_mesh, said_render_set_colormap and the said_render_read_* entries synchronise `stream`; said_render_render synchronises it
 * only when its workspace has to grow (a chunk longer than any before).
 */
#ifndef SAID_RENDER_H
#define SAID_RENDER_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_RENDER_MAX_K = 64, SAID_RENDER_MAX_LIGHTS = 4, SAID_RENDER_TILE = 32, SAID_RENDER_LUT = 256 };

/* Camera at cam_pos looking down -z with +y up (no rotation), pinhole intrinsics in pixels with cy measured from the top row; point lights
 * with 1 / d^2 fall-off; one metallic-roughness material for plain frames and one (base colour = vertex colour) for difference frames. */
typedef struct said_render_scene {
    int width, height;
    float fx, fy, cx, cy, znear, zfar;
    float cam_pos[3];
    int n_lights;
    float light_pos[SAID_RENDER_MAX_LIGHTS][3];
    float light_intensity[SAID_RENDER_MAX_LIGHTS];
    float ambient;
    float base_color[3];
    float metallic, roughness;       /* plain frames */
    float vc_metallic, vc_roughness; /* difference frames */
} said_render_scene;

typedef struct said_render said_render;
int said_render_create(said_render** out, int device);
int said_render_destroy(said_render* r);
const char* said_render_last_error(const said_render* r);

/* The mesh and its basis, replacing earlier ones: neutral_host (nv, 3) float64, faces_host (nf, 3) int32 vertex indices, blendshapes_host
 * (3 nv, k) float64 row-major, the columns b_1 .. b_k (not yet deltas: B_delta = B - n is formed here, in float64, and rounded to fp32 once).
 * The per-vertex incidence list of the normals kernel is built here, in ascending face index.  Fails, without touching the device, when
 * nf < 1, nv < 1, k outside 1 .. 64, a face index lies outside [0, nv) or a value is not finite.  Synchronises. */
int said_render_set_mesh(said_render* r, int nv, int nf, int k, const double* neutral_host, const int* faces_host, const double* blendshapes_host,
                         void* stream);
int said_render_set_scene(said_render* r, const said_render_scene* scene);
/* lut_host (256, 3) fp32 RGB in [0, 1]: the colour of difference bin i.  Synchronises. */
int said_render_set_colormap(said_render* r, const float* lut_host, void* stream);

/* Frames [t0, t0 + n_frames) of coeffs_dev (rows of k fp32 coefficients, at least t0 + n_frames of them) -> out_u8_dev (n_frames, height,
 * width, 3) uint8 in B, G, R order.  target_dev, nullable: the target sequence of the same shape; the frames then show
 * |B_delta (w' - w)| clipped to [0, max_diff] / max_diff through the colour map.  rot_host (3): axis-angle rotation applied about
 * t_center_host (3) before projection (NULL: none).  face_ids_dev, nullable: (n_frames, height, width) int32, the face drawn at each pixel,
 * -1 for background. */
int said_render_render(said_render* r, const float* coeffs_dev, const float* target_dev, long long t0, int n_frames, float max_diff,
                       const double* rot_host, const double* t_center_host, unsigned char* out_u8_dev, int* face_ids_dev, void* stream);

/* The stages of the last said_render_render, for its first n_frames frames: vertices before the rotation, their unit normals, and the
 * difference colours (zeros after a render without target), each (n_frames, nv, 3) fp32 into host memory.  Synchronise. */
int said_render_read_vertices(said_render* r, int n_frames, float* out_host, void* stream);
int said_render_read_normals(said_render* r, int n_frames, float* out_host, void* stream);
int said_render_read_colors(said_render* r, int n_frames, float* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_RENDER_H */
