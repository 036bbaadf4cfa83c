// jpeg_enc.cpp — host side of the JPEG encoder (C ABI: include/said_jpeg.h; kernels: jpeg.hip): the context, the
// tables of a configuration (typed in here: Annex K of the JPEG standard), the file header and the eight launches of a chunk.
#include "engine_internal.h"
#include "jpeg_kernels.h"
#include "../../include/said_jpeg.h"

using namespace said::jpeg;

struct said_jpeg {
    HostCtx c;
    bool configured = false;
    int quality = 0;
    Geom g{};
    Tables* tables = nullptr;            // device
    std::vector<unsigned char> header;   // SOI .. SOS
    // workspace of a chunk, grown on demand
    int cap = 0, last_n = 0;
    Work w{};
};

namespace {

// Annex K.1 quantisation tables in zigzag order, as a DQT segment carries them
const unsigned char QBASE[2][64] = {
    {16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29, 40, 58, 51, 61, 60, 57, 51,
     56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98, 103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99},
    {17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3 Huffman tables: codes per length 1 .. 16, then the symbols in code order
struct HuffSpec {
    unsigned char bits[16];
    int nvals;
    unsigned char vals[162];
};
const HuffSpec DC_SPEC[2] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}}};
const HuffSpec AC_SPEC[2] = {
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
      0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
      0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
      0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
      0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
      0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
      0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}}};

// natural index (vertical frequency * 8 + horizontal frequency) of every zigzag position: the anti-diagonals, alternately upwards and downwards
void zigzag_order(int* nat) {
    int i = 0;
    for (int s = 0; s < 15; ++s) {
        const int lo = std::max(0, s - 7), hi = std::min(s, 7);
        if (s % 2 == 0)
            for (int r = hi; r >= lo; --r) nat[i++] = r * 8 + (s - r);
        else
            for (int r = lo; r <= hi; ++r) nat[i++] = r * 8 + (s - r);
    }
}

// libjpeg's quality rule: s = 5000 / q below 50, else 200 - 2 q; entry = clamp((base s + 50) div 100, 1, 255)
int scaled_q(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    return std::min(255, std::max(1, (base * s + 50) / 100));
}

// canonical codes of a table: table[symbol] = code | length << 16
void derive_codes(const HuffSpec& h, unsigned* table) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < h.bits[len - 1]; ++i) table[h.vals[k++]] = code++ | ((unsigned)len << 16);
        code <<= 1;
    }
}

void put16(std::vector<unsigned char>& v, int x) {
    v.push_back((unsigned char)(x >> 8));
    v.push_back((unsigned char)(x & 0xFF));
}

void put_dht(std::vector<unsigned char>& v, int tc_th, const HuffSpec& h) {
    v.push_back(0xFF);
    v.push_back(0xC4);
    put16(v, 2 + 1 + 16 + h.nvals);
    v.push_back((unsigned char)tc_th);
    v.insert(v.end(), h.bits, h.bits + 16);
    v.insert(v.end(), h.vals, h.vals + h.nvals);
}

// SOI, APP0 (JFIF 1.01, no units, 1:1), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS
std::vector<unsigned char> make_header(int width, int height, const unsigned char (*qzz)[64]) {
    std::vector<unsigned char> v = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00, 0x01, 0x01, 0x00, 0x00, 0x01, 0x00, 0x01, 0x00, 0x00};
    for (int t = 0; t < 2; ++t) {
        v.insert(v.end(), {0xFF, 0xDB, 0x00, 0x43, (unsigned char)t});
        v.insert(v.end(), qzz[t], qzz[t] + 64);
    }
    v.insert(v.end(), {0xFF, 0xC0, 0x00, 0x11, 0x08});
    put16(v, height);
    put16(v, width);
    v.insert(v.end(), {0x03, 0x01, 0x22, 0x00, 0x02, 0x11, 0x01, 0x03, 0x11, 0x01});
    put_dht(v, 0x00, DC_SPEC[0]);
    put_dht(v, 0x10, AC_SPEC[0]);
    put_dht(v, 0x01, DC_SPEC[1]);
    put_dht(v, 0x11, AC_SPEC[1]);
    v.insert(v.end(), {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00});
    return v;
}

}  // namespace

extern "C" {

int said_jpeg_create(said_jpeg** out, int device) {
    DeviceRestore restore_device;
    said_jpeg* j = new_ctx("said_jpeg_create", out, device);
    if (!j) return -1;
    *out = j;
    return 0;
}

int said_jpeg_destroy(said_jpeg* j) { return delete_ctx(j); }

const char* said_jpeg_last_error(const said_jpeg* j) { return ctx_error(j); }

int said_jpeg_configure(said_jpeg* j, int width, int height, int quality) {
    if (!j) return -1;
    HostCtx* ctx = &j->c;
    j->configured = false;   // a refused configuration leaves none: the calls that need one say so
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(ctx, "said_jpeg_configure: image of %d x %d (1 .. 65535 each way)", width, height);
    if (quality < 1 || quality > 100) return fail(ctx, "said_jpeg_configure: quality %d (1 .. 100)", quality);
    const long long mcux = (width + 15) / 16, mcuy = (height + 15) / 16, nblocks = mcux * mcuy * BLOCKS_PER_MCU;
    if (nblocks > SAID_JPEG_MAX_BLOCKS)
        return fail(ctx, "said_jpeg_configure: %d x %d pads to %lld blocks of 8 x 8, more than %d (a frame's bit offsets are 32-bit)", width, height, nblocks, (int)SAID_JPEG_MAX_BLOCKS);
    Tables t{};
    int nat[64];
    zigzag_order(nat);
    unsigned char qzz[2][64];
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            qzz[c][i] = (unsigned char)scaled_q(QBASE[c][i], quality);
            t.q[c][nat[i]] = (float)qzz[c][i];
        }
    for (int i = 0; i < 64; ++i) t.zz[nat[i]] = (unsigned char)i;
    const double pi = 3.14159265358979323846;
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) t.basis[u * 8 + x] = (float)(std::sqrt((u == 0 ? 1.0 : 2.0) / 8.0) * std::cos((2 * x + 1) * u * pi / 16.0));
    for (int c = 0; c < 2; ++c) {
        derive_codes(DC_SPEC[c], t.dc[c]);
        derive_codes(AC_SPEC[c], t.ac[c]);
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    j->cap = j->last_n = 0;   // the workspace is sized by the image
    if (!j->tables && dalloc(ctx, &j->tables, 1, false)) return -1;
    HIPCHK(hipMemcpy(j->tables, &t, sizeof(Tables), hipMemcpyHostToDevice));
    Geom g{};
    g.width = width;
    g.height = height;
    g.mcux = (int)mcux;
    g.mcuy = (int)mcuy;
    g.nblocks = (int)nblocks;
    // the worst-case stream of a frame and up to seven padding bits, in whole pieces
    const long long words = (nblocks * MAX_BLOCK_BITS + 7 + 31) / 32;
    g.pieces = (int)((words + PIECE_WORDS - 1) / PIECE_WORDS);
    g.stride_words = (unsigned)g.pieces * PIECE_WORDS;
    j->g = g;
    j->quality = quality;
    j->header = make_header(width, height, qzz);
    j->configured = true;
    return 0;
}

int said_jpeg_header(said_jpeg* j, unsigned char* out_host, long long capacity, long long* size_host) {
    if (!j) return -1;
    HostCtx* ctx = &j->c;
    if (!j->configured) return fail(ctx, "said_jpeg_header: not configured (said_jpeg_configure)");
    const long long n = (long long)j->header.size();
    if (size_host) *size_host = n;
    if (!out_host || capacity < n) return fail(ctx, "said_jpeg_header: the header takes %lld bytes, the buffer has %lld", n, out_host ? capacity : 0LL);
    std::memcpy(out_host, j->header.data(), (size_t)n);
    return 0;
}

int said_jpeg_encode(said_jpeg* j, const unsigned char* frames_dev, int n_frames, int bgr, unsigned char* out_dev, long long capacity,
                     long long* offsets_dev, long long* required_host, void* stream) {
    if (!j) return -1;
    HostCtx* ctx = &j->c;
    if (!j->configured) return fail(ctx, "said_jpeg_encode: not configured (said_jpeg_configure)");
    if (!frames_dev || !offsets_dev || !required_host) return fail(ctx, "said_jpeg_encode: null frames, offsets or required");
    if (n_frames < 1 || n_frames > SAID_JPEG_MAX_FRAMES) return fail(ctx, "said_jpeg_encode: n_frames %d (1 .. %d frames per call)", n_frames, (int)SAID_JPEG_MAX_FRAMES);
    if (capacity < 0 || (capacity > 0 && !out_dev)) return fail(ctx, "said_jpeg_encode: capacity %lld with %s output buffer", capacity, out_dev ? "an" : "no");
    const Geom& g = j->g;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (n_frames > j->cap) {
        HIPCHK(hipStreamSynchronize(s));
        j->cap = j->last_n = 0;
        const size_t n = (size_t)n_frames;
        if (drealloc(ctx, &j->w.coef, n * g.nblocks * 64, false) || drealloc(ctx, &j->w.bits, n * g.nblocks, false) || drealloc(ctx, &j->w.words, n * g.stride_words, false) ||
            drealloc(ctx, &j->w.piece, n * g.pieces, false) || drealloc(ctx, &j->w.total_bits, n, false) || drealloc(ctx, &j->w.total_bytes, n, false))
            return -1;
        j->cap = n_frames;
    }
    const Work& w = j->w;
    j->last_n = 0;
    HIPCHK(hipMemsetAsync(w.words, 0, sizeof(unsigned) * (size_t)n_frames * g.stride_words, s));
    launch_transform(frames_dev, n_frames, bgr != 0, g, j->tables, w, s);
    HIPCHK(hipGetLastError());
    launch_block_bits(n_frames, g, j->tables, w, s);
    HIPCHK(hipGetLastError());
    launch_scan(w.bits, g.nblocks, w.total_bits, n_frames, s);
    HIPCHK(hipGetLastError());
    launch_pack(n_frames, g, j->tables, w, s);
    HIPCHK(hipGetLastError());
    launch_count_stuffed(n_frames, g, w, s);
    HIPCHK(hipGetLastError());
    launch_scan(w.piece, g.pieces, w.total_bytes, n_frames, s);
    HIPCHK(hipGetLastError());
    launch_offsets(n_frames, w, offsets_dev, s);
    HIPCHK(hipGetLastError());
    launch_stuff(n_frames, g, w, offsets_dev, out_dev, capacity, s);
    HIPCHK(hipGetLastError());
    long long total = 0;
    HIPCHK(hipMemcpyAsync(&total, offsets_dev + n_frames, sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    j->last_n = n_frames;
    *required_host = total;
    return total > capacity ? SAID_JPEG_OVERFLOW : 0;
}

int said_jpeg_read_coefficients(said_jpeg* j, int n_frames, short* out_host, void* stream) {
    if (!j) return -1;
    HostCtx* ctx = &j->c;
    if (!out_host || n_frames < 1 || n_frames > j->last_n)
        return fail(ctx, "said_jpeg_read_coefficients: n_frames %d outside 1 .. %d (the last encode's chunk)", n_frames, j->last_n);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out_host, j->w.coef, sizeof(short) * 64 * (size_t)j->g.nblocks * n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
