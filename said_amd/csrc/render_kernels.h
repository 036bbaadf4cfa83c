// render_kernels.h — launchers of render.hip for renderer.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/said_render.h"

namespace said {
namespace render __attribute__((visibility("hidden"))) {

constexpr int TRI_REC = 12;    // floats per triangle record: sx0 sy0 sx1 sy1 sx2 sy2 1/d0 1/d1 1/d2 id - -
constexpr int TRI_ATTR = 27;   // floats per triangle attribute block: 3 positions, 3 normals, 3 colours (vertex order of the record)

struct Mesh {
    int nv, nf, k;
    const float* neutral;   // (nv, 3)
    const float* bdelta;    // (k, nv, 3)
    const int* faces;       // (nf, 3)
    const float* nedge;     // (nf, 12): the neutral's edges n1 - n0, n2 - n0 of every face, formed in float64: 6 fp32 hi parts, 6 lo parts
    const float* ebasis;    // (k, nf, 12): the same two edges of every B_delta[k], split the same way
    const int* inc_off;     // (nv + 1)
    const int* inc;         // face * 4 + corner, ascending face index per vertex
};

struct Frames {   // the workspace of one chunk
    int n;
    float* verts;     // (n, nv, 3)
    float* face_na;   // (n, nf, 6): unit face normal, the three corner angles
    float* normals;   // (n, nv, 3)
    float* colors;    // (n, nv, 3)
    float* tri_rec;   // (n, nf, TRI_REC)
    int* tri_box;     // (n, nf, 2): xmin | xmax << 16, ymin | ymax << 16 (empty: xmin > xmax)
    float* tri_attr;  // (n, nf, TRI_ATTR)
};

struct Xform {
    float R[9];   // row-major
    float c[3];
};

void launch_blend_vertices(const Mesh& m, const Frames& f, const float* coeffs, const float* target, float max_diff, const float* lut, hipStream_t s);
void launch_face_normals(const Mesh& m, const Frames& f, const float* coeffs, hipStream_t s);
void launch_vertex_normals(const Mesh& m, const Frames& f, hipStream_t s);
void launch_tri_setup(const Mesh& m, const Frames& f, const said_render_scene& sc, const Xform& x, bool vertex_colors, hipStream_t s);
void launch_raster_shade(const Mesh& m, const Frames& f, const said_render_scene& sc, bool vertex_colors, unsigned char* out, int* face_ids,
                         hipStream_t s);
// 4 samples per pixel; sample_ids (n, height, width, 4), 16-byte aligned, nullable
void launch_raster_shade_ms(const Mesh& m, const Frames& f, const said_render_scene& sc, bool vertex_colors, unsigned char* out, int* sample_ids,
                            hipStream_t s);

}  // namespace render
}  // namespace said
