/*
 * said_jpeg.h — C ABI of the baseline JPEG encoder (said_amd/csrc/jpeg.hip, jpeg_enc.cpp), in libsaid_hip.so beside said_render.h.
 *
 * The renderer leaves its frames on the device as (n, height, width, 3) uint8.  This context turns each of them into one baseline sequential
 * JFIF file without a trip through the host: SOF0, 8 bits, Y at 2x2 and Cb, Cr at 1x1 sampling (4:2:0), one interleaved scan, the Annex K
 * quantisation tables scaled by libjpeg's quality rule and the four Annex K Huffman tables, no restart markers.  DESIGN.md section 15.1 is
 * the specification: sample formulas, transform, rounding and entropy coding, symbol by symbol.
 *
 * A file is the header (SOI through SOS, said_jpeg_header: the same bytes for every frame of a configuration) followed by the frame's scan
 * and EOI, which said_jpeg_encode writes for all frames of a call back to back into one device buffer, with (n + 1) offsets beside it.
 *
 * Conventions are those of said_render.h: 0 on success, said_jpeg_last_error(ctx) (NULL for create failures) gives the message; `*_dev` are
 * device pointers, `*_host` host memory; `stream` is a hipStream_t.  Nothing aborts.  The transform is fp32 in fixed-order chains and
 * everything after it is integer arithmetic (bits are only ever OR-ed into zeroed words): a frame's bytes do not depend on the chunk it is
 * encoded in, and equal inputs give identical bytes.
 */
#ifndef SAID_JPEG_H
#define SAID_JPEG_H

#ifdef __cplusplus
extern "C" {
#endif

/* said_jpeg_encode's result when the output does not fit its buffer (not an error: last_error is not set) */
enum { SAID_JPEG_OVERFLOW = 1, SAID_JPEG_MAX_FRAMES = 4096, SAID_JPEG_MAX_BLOCKS = 1000000 };

typedef struct said_jpeg said_jpeg;
int said_jpeg_create(said_jpeg** out, int device);
int said_jpeg_destroy(said_jpeg* j);
const char* said_jpeg_last_error(const said_jpeg* j);

/* Image size and quality of the calls that follow.  Fails, with a message, when width or height is below 1 or above 65535, when the padded
 * image has more than SAID_JPEG_MAX_BLOCKS 8 x 8 blocks (six per 16 x 16 pixels; a frame's bit offsets are 32-bit), or when quality lies
 * outside 1 .. 100; the context is then without a configuration until a later call succeeds.  Synchronises the device. */
int said_jpeg_configure(said_jpeg* j, int width, int height, int quality);

/* The bytes from SOI through SOS into out_host; *size_host receives their number (623) also when capacity is too small, which fails. */
int said_jpeg_header(said_jpeg* j, unsigned char* out_host, long long capacity, long long* size_host);

/* frames_dev (n_frames, height, width, 3) uint8, B G R when bgr is non-zero and R G B otherwise -> out_dev: for each frame its entropy-coded
 * scan followed by EOI, frames back to back; offsets_dev receives (n_frames + 1) int64 offsets into out_dev, the last being the total.
 * *required_host receives that total.  When it exceeds `capacity` (the bytes of out_dev) nothing is written at or past out_dev + capacity,
 * the bytes before it are unspecified, the offsets are still those of the full output and the result is SAID_JPEG_OVERFLOW.
 * Synchronises `stream` once, after all its kernels are enqueued, to learn the total (and before them when the workspace has to grow). */
int said_jpeg_encode(said_jpeg* j, const unsigned char* frames_dev, int n_frames, int bgr, unsigned char* out_dev, long long capacity,
                     long long* offsets_dev, long long* required_host, void* stream);

/* The quantised coefficients of the last said_jpeg_encode, for its first n_frames frames: (n_frames, blocks, 64) int16 into host memory,
 * blocks in scan order (MCU by MCU: Y00 Y01 Y10 Y11 Cb Cr), each in zigzag order.  Synchronises. */
int said_jpeg_read_coefficients(said_jpeg* j, int n_frames, short* out_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_JPEG_H */
