/*
 * said_render_ms.h — the renderer's multisampled entry point (said_amd/csrc/render.hip, renderer.cpp), in libsaid_hip.so beside
 * said_render.h, whose contexts, scene, mesh and conventions it uses.  DESIGN.md section 15.2 is the specification.
 *
 * pyrender draws into a 4-sample multisampled framebuffer and blits it down to one sample; said_render_render takes one sample per pixel.
 * With samples = 4 this entry tests coverage and depth at four positions per pixel, at these offsets from the pixel centre (x right, y down):
 *     s0 = (-0.125, -0.375)   s1 = (+0.375, -0.125)   s2 = (-0.375, +0.125)   s3 = (+0.125, +0.375)
 * shades each distinct face among a pixel's four winners once, at the pixel centre, quantises that colour to 8 bits and stores per channel
 * (c0 + c1 + c2 + c3 + 2) >> 2, a sample that nothing covers counting as 0.  A pixel whose four samples show the face said_render_render
 * draws there gets that render's bytes exactly.
 */
#ifndef SAID_RENDER_MS_H
#define SAID_RENDER_MS_H

#include "said_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* said_render_render with the sample count as an argument: 1 or 4, anything else is an error before any launch.
 * samples == 1: the path of said_render_render, with its outputs bit for bit; sample_ids_dev must be NULL.
 * samples == 4: out_u8_dev gets the resolved frames; face_ids_dev must be NULL; sample_ids_dev, nullable and 16-byte aligned: (n_frames,
 * height, width, 4) int32, the face of each sample in the order above, -1 for none.
 * Every other argument, the validation, the stream behaviour and the said_render_read_* stage readers are those of said_render_render. */
int said_render_render_ms(said_render* r, int samples, const float* coeffs_dev, const float* target_dev, long long t0, int n_frames,
                          float max_diff, const double* rot_host, const double* t_center_host, unsigned char* out_u8_dev, int* face_ids_dev,
                          int* sample_ids_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_RENDER_MS_H */
