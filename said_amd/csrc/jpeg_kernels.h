// jpeg_kernels.h — launchers of jpeg.hip for jpeg_enc.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace jpeg __attribute__((visibility("hidden"))) {

constexpr int BLOCKS_PER_MCU = 6;       // Y00 Y01 Y10 Y11 Cb Cr
// the longest code sequence of one block: DC 11 + 11 bits, 63 AC coefficients of 16 + 10 bits each (a zero run only shortens it)
constexpr int MAX_BLOCK_BITS = 22 + 63 * 26;
constexpr int PIECE = 128;              // bytes of the unstuffed stream one thread of the byte-stuffing kernels handles
constexpr int PIECE_WORDS = PIECE / 4;

struct Tables {               // one device copy per configuration
    float basis[64];          // basis[u * 8 + x] = C(u) cos((2 x + 1) u pi / 16), formed in float64 and rounded once
    float q[2][64];           // quantisation steps in natural order (vertical frequency * 8 + horizontal frequency)
    unsigned dc[2][12];       // Huffman code | length << 16 of every size category
    unsigned ac[2][256];      // of every run << 4 | size symbol (0 where the table has none)
    unsigned char zz[64];     // zigzag position of a natural index
};

struct Geom {
    int width, height, mcux, mcuy;
    int nblocks;              // blocks per frame, in scan order
    unsigned stride_words;    // 32-bit words of unstuffed stream reserved per frame (worst case; a multiple of PIECE_WORDS)
    int pieces;               // stride_words / PIECE_WORDS
};

struct Work {                 // the workspace of one call, per frame
    short* coef;              // (n, nblocks, 64) zigzag order
    unsigned* bits;           // (n, nblocks): bits of each block, then (after the scan) its bit offset in the frame's stream
    unsigned* words;          // (n, stride_words): the unstuffed stream, most significant bit first
    unsigned* piece;          // (n, pieces): output bytes of each piece, then its byte offset in the frame's output
    unsigned* total_bits;     // (n)
    unsigned* total_bytes;    // (n): stuffed bytes of the scan, without EOI
};

void launch_transform(const unsigned char* frames, int n, bool bgr, const Geom& g, const Tables* t, const Work& w, hipStream_t s);
void launch_block_bits(int n, const Geom& g, const Tables* t, const Work& w, hipStream_t s);
void launch_scan(unsigned* data, int count, unsigned* totals, int n, hipStream_t s);
void launch_pack(int n, const Geom& g, const Tables* t, const Work& w, hipStream_t s);
void launch_count_stuffed(int n, const Geom& g, const Work& w, hipStream_t s);
void launch_offsets(int n, const Work& w, long long* offsets, hipStream_t s);
void launch_stuff(int n, const Geom& g, const Work& w, const long long* offsets, unsigned char* out, long long capacity, hipStream_t s);

}  // namespace jpeg
}  // namespace said
