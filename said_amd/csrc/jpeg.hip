// jpeg.hip — the baseline JPEG encoder's kernels (C ABI: include/said_jpeg.h; host side: jpeg_enc.cpp; specification: DESIGN.md section 15.1).
//
// Eight launches per chunk of frames, every one with the frame in blockIdx.y (or blockIdx.x for the per-frame scans), so a frame's bytes
// never depend on the chunk it is in:
//   transform_kernel      one workgroup per 16 x 16 MCU: colour conversion, chroma means, row and column DCT through LDS, quantisation;
//                         int16 coefficients in zigzag order, blocks in scan order
//   block_bits_kernel     bits each block will emit, from its coefficients and its predecessor's DC                 one thread per block
//   scan_kernel           exclusive prefix sum per frame (block bits -> bit offsets; later piece bytes -> byte offsets)  one workgroup per frame
//   pack_kernel           every block writes its codes at its bit offset into the zeroed word stream; the first and last word of a block
//                         are shared with its neighbours and combined by atomicOr (bits only ever set: exact)        one thread per block
//   count_stuffed_kernel  output bytes of every 128-byte piece of the stream: its bytes plus its 0xFF bytes             one thread per piece
//   offsets_kernel        the (n + 1) int64 offsets of the frames in the output                                        one thread
//   stuff_kernel          copies a piece with a 0x00 after every 0xFF, every store guarded by the capacity; piece 0 appends EOI
// The transform is fp32 in fixed-order fmaf chains (the library is built with -ffp-contract=off, so nothing else is fused); everything after
// it is integer arithmetic.
#include "jpeg_kernels.h"

namespace said {
namespace jpeg {

namespace {

// ---- transform
__global__ __launch_bounds__(256) void transform_kernel(const unsigned char* __restrict__ frames, int bgr, Geom g, const Tables* __restrict__ t,
                                                        short* __restrict__ coef) {
    __shared__ float blk[BLOCKS_PER_MCU][8][9], tmp[BLOCKS_PER_MCU][8][9], cb[16][17], cr[16][17], basis[64], q[2][64];
    __shared__ unsigned char zz[64];
    __shared__ short outc[BLOCKS_PER_MCU * 64];
    const int tid = threadIdx.x, fr = blockIdx.y, mcu = blockIdx.x;
    const int my = mcu / g.mcux, mx = mcu - my * g.mcux;
    if (tid < 64) {
        basis[tid] = t->basis[tid];
        zz[tid] = t->zz[tid];
    } else if (tid < 192) {
        q[(tid - 64) >> 6][(tid - 64) & 63] = t->q[(tid - 64) >> 6][(tid - 64) & 63];
    }
    {
        const int y = tid >> 4, x = tid & 15;
        const int py = min(my * 16 + y, g.height - 1), px = min(mx * 16 + x, g.width - 1);   // the last row and column are replicated
        const unsigned char* p = frames + (((size_t)fr * g.height + py) * g.width + px) * 3;
        const float c0 = (float)p[0], G = (float)p[1], c2 = (float)p[2];
        const float R = bgr ? c2 : c0, B = bgr ? c0 : c2;
        blk[(y >> 3) * 2 + (x >> 3)][y & 7][x & 7] = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R)) - 128.0f;
        cb[y][x] = fmaf(0.5f, B, fmaf(-0.331264108f, G, -0.168735892f * R));
        cr[y][x] = fmaf(-0.081312411f, B, fmaf(-0.418687589f, G, 0.5f * R));
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 6, y = (tid >> 3) & 7, x = tid & 7;
        const float(*s)[17] = c ? cr : cb;
        blk[4 + c][y][x] = ((s[2 * y][2 * x] + s[2 * y][2 * x + 1]) + (s[2 * y + 1][2 * x] + s[2 * y + 1][2 * x + 1])) * 0.25f;
    }
    __syncthreads();
    for (int o = tid; o < BLOCKS_PER_MCU * 64; o += 256) {   // rows: tmp[k][r][u] = sum_x blk[k][r][x] basis[u][x]
        const int k = o >> 6, r = (o >> 3) & 7, u = o & 7;
        float a = blk[k][r][0] * basis[u * 8];
#pragma unroll
        for (int x = 1; x < 8; ++x) a = fmaf(blk[k][r][x], basis[u * 8 + x], a);
        tmp[k][r][u] = a;
    }
    __syncthreads();
    for (int o = tid; o < BLOCKS_PER_MCU * 64; o += 256) {   // columns: F[k][v][u] = sum_y tmp[k][y][u] basis[v][y]
        const int k = o >> 6, v = (o >> 3) & 7, u = o & 7;
        float a = tmp[k][0][u] * basis[v * 8];
#pragma unroll
        for (int y = 1; y < 8; ++y) a = fmaf(tmp[k][y][u], basis[v * 8 + y], a);
        const int nat = v * 8 + u;
        const float m = floorf(fabsf(a) / q[k >> 2][nat] + 0.5f);   // sign(F) floor(|F| / Q + 0.5)
        int iv = (int)fminf(m, 1024.0f);
        if (a < 0.0f) iv = -iv;
        // |F| <= 1024 for DC and < 1021 for AC with samples in [-128, 127]; the clamp keeps every value inside the Huffman tables' categories
        iv = nat == 0 ? max(-1024, min(iv, 1023)) : max(-1023, min(iv, 1023));
        outc[k * 64 + zz[nat]] = (short)iv;
    }
    __syncthreads();
    short* dst = coef + ((size_t)fr * g.nblocks + (size_t)mcu * BLOCKS_PER_MCU) * 64;
    for (int o = tid; o < BLOCKS_PER_MCU * 64; o += 256) dst[o] = outc[o];
}

// ---- entropy coding: one walk over a block's coefficients, shared by the bit count and the packer
// DC of the previous block of the same component in scan order (0 at the start of a frame)
__device__ __forceinline__ int dc_predictor(const short* __restrict__ frame_coef, int b) {
    const int m = b / BLOCKS_PER_MCU, k = b - m * BLOCKS_PER_MCU;
    if (k >= 1 && k <= 3) return frame_coef[(size_t)(b - 1) * 64];
    if (m == 0) return 0;
    return frame_coef[(size_t)(k == 0 ? b - 3 : b - BLOCKS_PER_MCU) * 64];
}

__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }   // 0 for v == 0
// the s value bits of v: v itself, or v + 2^s - 1 when negative
__device__ __forceinline__ unsigned value_bits(int v, int s) { return (unsigned)(v - (v < 0 ? 1 : 0)) & ((1u << s) - 1u); }

template <class Sink>
__device__ __forceinline__ void code_block(const short* __restrict__ c, int pred, const unsigned* dc, const unsigned* ac, Sink& sink) {
    const int4* c4 = reinterpret_cast<const int4*>(c);   // 64 int16 = 8 x 16 bytes, 128-byte aligned
    int run = 0;
    for (int j = 0; j < 8; ++j) {
        const int4 v4 = c4[j];
        const int w[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = (int)(short)((unsigned)w[e >> 1] >> ((e & 1) * 16));
            if (e == 0 && j == 0) {
                const int d = v - pred, s = category(d);
                const unsigned h = dc[s];
                sink.put(((h & 0xFFFFu) << s) | value_bits(d, s), (int)(h >> 16) + s);
                continue;
            }
            if (v == 0) {
                ++run;
                continue;
            }
            while (run > 15) {
                const unsigned h = ac[0xF0];   // ZRL
                sink.put(h & 0xFFFFu, (int)(h >> 16));
                run -= 16;
            }
            const int s = category(v);
            const unsigned h = ac[(run << 4) | s];
            sink.put(((h & 0xFFFFu) << s) | value_bits(v, s), (int)(h >> 16) + s);
            run = 0;
        }
    }
    if (run > 0) {
        const unsigned h = ac[0x00];   // EOB
        sink.put(h & 0xFFFFu, (int)(h >> 16));
    }
}

struct CountSink {
    unsigned n = 0;
    __device__ __forceinline__ void put(unsigned, int len) { n += (unsigned)len; }
};

// Appends codes of at most 32 bits to a stream of big-endian 32-bit words starting at any bit offset.  The first word it touches and the word
// it leaves unfinished are shared with the neighbouring blocks: those are OR-ed in atomically; the words between are this block's alone.
struct WordSink {
    unsigned* words;
    unsigned limit;           // words of the frame's stream
    unsigned w;               // index of the word being filled
    int cnt;                  // bits of it already accounted for (the offset's bits inside the first word count as zeros)
    unsigned long long acc = 0;
    bool first = true;
    __device__ __forceinline__ WordSink(unsigned* words_, unsigned limit_, unsigned bit_offset) : words(words_), limit(limit_), w(bit_offset >> 5), cnt((int)(bit_offset & 31u)) {}
    __device__ __forceinline__ void put(unsigned code, int len) {
        acc = (acc << len) | code;
        cnt += len;
        if (cnt >= 32) {
            cnt -= 32;
            const unsigned word = (unsigned)(acc >> cnt);
            if (w < limit) {
                if (first) atomicOr(words + w, word);
                else words[w] = word;
            }
            first = false;
            ++w;
        }
    }
    __device__ __forceinline__ void flush() {
        if (cnt > 0 && w < limit) atomicOr(words + w, (unsigned)(acc << (32 - cnt)));
    }
};

__device__ __forceinline__ void load_huffman(const Tables* __restrict__ t, unsigned (*dc)[12], unsigned (*ac)[256]) {
    for (int i = threadIdx.x; i < 512; i += blockDim.x) ac[i >> 8][i & 255] = t->ac[i >> 8][i & 255];
    if (threadIdx.x < 24) dc[threadIdx.x / 12][threadIdx.x % 12] = t->dc[threadIdx.x / 12][threadIdx.x % 12];
    __syncthreads();
}

__global__ __launch_bounds__(256) void block_bits_kernel(const short* __restrict__ coef, Geom g, const Tables* __restrict__ t, unsigned* __restrict__ bits) {
    __shared__ unsigned dc[2][12], ac[2][256];
    load_huffman(t, dc, ac);
    const int b = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (b >= g.nblocks) return;
    const short* fc = coef + (size_t)fr * g.nblocks * 64;
    const int tab = (b % BLOCKS_PER_MCU) >= 4 ? 1 : 0;
    CountSink sink;
    code_block(fc + (size_t)b * 64, dc_predictor(fc, b), dc[tab], ac[tab], sink);
    bits[(size_t)fr * g.nblocks + b] = sink.n;
}

__global__ __launch_bounds__(256) void pack_kernel(const short* __restrict__ coef, Geom g, const Tables* __restrict__ t, const unsigned* __restrict__ bit_offset,
                                                   unsigned* __restrict__ words) {
    __shared__ unsigned dc[2][12], ac[2][256];
    load_huffman(t, dc, ac);
    const int b = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (b >= g.nblocks) return;
    const short* fc = coef + (size_t)fr * g.nblocks * 64;
    const int tab = (b % BLOCKS_PER_MCU) >= 4 ? 1 : 0;
    WordSink sink(words + (size_t)fr * g.stride_words, g.stride_words, bit_offset[(size_t)fr * g.nblocks + b]);
    code_block(fc + (size_t)b * 64, dc_predictor(fc, b), dc[tab], ac[tab], sink);
    if (b == g.nblocks - 1) {   // the frame's last byte is padded with 1 bits
        const int pad = (8 - (sink.cnt & 7)) & 7;
        if (pad) sink.put((1u << pad) - 1u, pad);
    }
    sink.flush();
}

// ---- exclusive prefix sum of `count` values per frame, in place; the sum goes to totals[frame]
__global__ __launch_bounds__(1024) void scan_kernel(unsigned* __restrict__ data, int count, unsigned* __restrict__ totals) {
    __shared__ unsigned wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* d = data + (size_t)blockIdx.x * count;
    unsigned carry = 0;
    for (int base = 0; base < count; base += 1024) {
        const int i = base + tid;
        const unsigned v = i < count ? d[i] : 0u;
        unsigned x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned s = wsum[k];
            before += k < wave ? s : 0u;
            all += s;
        }
        if (i < count) d[i] = carry + before + x - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

// ---- byte stuffing
__device__ __forceinline__ unsigned count_ff(unsigned w) {
    return (unsigned)((w >> 24) == 0xFFu) + (unsigned)(((w >> 16) & 0xFFu) == 0xFFu) + (unsigned)(((w >> 8) & 0xFFu) == 0xFFu) + (unsigned)((w & 0xFFu) == 0xFFu);
}

__global__ __launch_bounds__(256) void count_stuffed_kernel(const unsigned* __restrict__ words, const unsigned* __restrict__ total_bits, Geom g,
                                                            unsigned* __restrict__ piece) {
    const int p = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (p >= g.pieces) return;
    const unsigned nbytes = (total_bits[fr] + 7u) >> 3, start = (unsigned)p * PIECE;
    unsigned n = 0;
    if (start < nbytes) {
        const unsigned len = min((unsigned)PIECE, nbytes - start);
        n = len;
        const uint4* src = reinterpret_cast<const uint4*>(words + (size_t)fr * g.stride_words + (size_t)p * PIECE_WORDS);
        // whole words: the bytes after the stream's end are zero, never 0xFF
        for (int i = 0; i < PIECE_WORDS / 4 && (unsigned)i * 16u < len; ++i) {
            const uint4 v = src[i];
            n += count_ff(v.x) + count_ff(v.y) + count_ff(v.z) + count_ff(v.w);
        }
    }
    piece[(size_t)fr * g.pieces + p] = n;
}

__global__ void offsets_kernel(const unsigned* __restrict__ total_bytes, int n, long long* __restrict__ offsets) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long o = 0;
    offsets[0] = 0;
    for (int f = 0; f < n; ++f) {
        o += (long long)total_bytes[f] + 2;   // the scan and EOI
        offsets[f + 1] = o;
    }
}

__global__ __launch_bounds__(256) void stuff_kernel(const unsigned* __restrict__ words, const unsigned* __restrict__ total_bits,
                                                    const unsigned* __restrict__ piece_offset, const long long* __restrict__ offsets, Geom g,
                                                    unsigned char* __restrict__ out, long long capacity) {
    const int p = blockIdx.x * 256 + threadIdx.x, fr = blockIdx.y;
    if (p >= g.pieces) return;
    if (p == 0) {   // EOI closes the frame
        const long long e = offsets[fr + 1];
        if (e - 2 >= 0 && e - 2 < capacity) out[e - 2] = 0xFF;
        if (e - 1 >= 0 && e - 1 < capacity) out[e - 1] = 0xD9;
    }
    const unsigned nbytes = (total_bits[fr] + 7u) >> 3, start = (unsigned)p * PIECE;
    if (start >= nbytes) return;
    const unsigned n = min((unsigned)PIECE, nbytes - start);
    const unsigned* src = words + (size_t)fr * g.stride_words + (size_t)p * PIECE_WORDS;
    long long pos = offsets[fr] + (long long)piece_offset[(size_t)fr * g.pieces + p];
    for (unsigned i = 0; i < n; i += 4) {
        const unsigned w = src[i >> 2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < n) {
                const unsigned char byte = (unsigned char)(w >> (24 - 8 * k));
                if (pos < capacity) out[pos] = byte;
                ++pos;
                if (byte == 0xFF) {
                    if (pos < capacity) out[pos] = 0x00;
                    ++pos;
                }
            }
        }
    }
}

inline dim3 per_item(int items, int n) { return dim3((unsigned)((items + 255) / 256), (unsigned)n); }

}  // namespace

void launch_transform(const unsigned char* frames, int n, bool bgr, const Geom& g, const Tables* t, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)(g.mcux * g.mcuy), (unsigned)n), dim3(256), 0, s, frames, bgr ? 1 : 0, g, t, w.coef);
}
void launch_block_bits(int n, const Geom& g, const Tables* t, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(block_bits_kernel, per_item(g.nblocks, n), dim3(256), 0, s, w.coef, g, t, w.bits);
}
void launch_scan(unsigned* data, int count, unsigned* totals, int n, hipStream_t s) {
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n), dim3(1024), 0, s, data, count, totals);
}
void launch_pack(int n, const Geom& g, const Tables* t, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(pack_kernel, per_item(g.nblocks, n), dim3(256), 0, s, w.coef, g, t, w.bits, w.words);
}
void launch_count_stuffed(int n, const Geom& g, const Work& w, hipStream_t s) {
    hipLaunchKernelGGL(count_stuffed_kernel, per_item(g.pieces, n), dim3(256), 0, s, w.words, w.total_bits, g, w.piece);
}
void launch_offsets(int n, const Work& w, long long* offsets, hipStream_t s) {
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, s, w.total_bytes, n, offsets);
}
void launch_stuff(int n, const Geom& g, const Work& w, const long long* offsets, unsigned char* out, long long capacity, hipStream_t s) {
    hipLaunchKernelGGL(stuff_kernel, per_item(g.pieces, n), dim3(256), 0, s, w.words, w.total_bits, w.piece, offsets, g, out, capacity);
}

}  // namespace jpeg
}  // namespace said
