// trsim_jpeg.hip — the tub image encoder: uint8[n][H][W][3] frames on the device -> baseline JPEG files (quality q, 4:2:0, the standard's Huffman
// tables), byte for byte what include/trsim_spec.h ("tub image (JPEG)") defines.  Every table and every arithmetic rule comes from
// trsim_jpeg_tables.hpp, the stage from raw rows to sample planes from trsim_jpeg_device.hpp; this file holds the rest of the data movement:
// trs_jpeg_kernel (frames -> one slot of `cap` bytes per frame + its length) and
// trs_jpeg_pack_kernel (slots -> the files back to back + their offsets, for the one device-to-host copy of trs_encode_jpeg_host).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_jpeg_device.hpp"
#include "trsim_jpeg_host.hpp"

namespace {
namespace jpeg = trsim::jpeg;

struct JpegParams {
    const uint8_t* src;          // uint8[n][H][W][3], 4-byte aligned
    uint8_t* dst;                // n slots of cap bytes
    int32_t* len;                // int32[n]
    const jpeg::Tables* tab;
    int n, H, W, cap;
    jpeg::StripeLds lds;
};

extern __shared__ __attribute__((aligned(16))) unsigned char jsmem[];

// exclusive prefix sum of one value per thread over the workgroup's 256 threads; *total: the sum.  scratch: 4 ints of LDS
__device__ int block_scan(int v, int* scratch, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();                                    // the scratch words of the scan before this one have been read
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < jpeg::kThreads / 64; ++w) {
        const int s = scratch[w];
        if (w < wave) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// byte j of the bit stream, which is kept as dwords whose most significant bit comes first
__device__ inline uint32_t stream_byte(const uint32_t* s, int j) { return (s[j >> 2] >> (24 - 8 * (j & 3))) & 255u; }

// One workgroup per frame at a time, one MCU row (16 image rows) at a time:
//   raw RGB rows -> LDS | colour + 2x2 downsampling -> sample planes | DCT rows | DCT columns + quantiser -> blocks in zig-zag order |
//   one lane per block: code length, workgroup prefix sum, codes ORed into the zeroed bit stream | 0xFF count + prefix sum | stuffed bytes -> the slot.
// Carried from one MCU row to the next: the three DC predictors, the bits of the last partial byte, the slot offset.
__global__ __launch_bounds__(jpeg::kThreads) void trs_jpeg_kernel(JpegParams p)
{
    const jpeg::Geometry g = jpeg::geometry(p.H, p.W);
    const int tid = threadIdx.x, mw = g.mcu_cols, nb = jpeg::blocks_per_stripe(g);
    jpeg::Tables* T = reinterpret_cast<jpeg::Tables*>(jsmem + p.lds.off_tab);
    uint8_t* ys = jsmem + p.lds.off_y;                                   // [16][16 mw]
    uint8_t* cs = jsmem + p.lds.off_c;                                   // [2][8][8 mw]
    uint32_t* ws = reinterpret_cast<uint32_t*>(jsmem + p.lds.off_ws);    // raw rows, then int32[nb][8][8] between the DCT passes, then the bit stream
    int16_t* coef = reinterpret_cast<int16_t*>(jsmem + p.lds.off_coef);  // [nb][kCoefStride], zig-zag order
    int* scan = reinterpret_cast<int*>(jsmem + p.lds.off_scan);
    const int ws_dwords = nb * 64 + 4, ystride = 16 * mw, cstride = 8 * mw, row_bytes = p.W * 3;
    {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(p.tab);
        uint32_t* d = reinterpret_cast<uint32_t*>(T);
        for (int i = tid; i < (int)(sizeof(jpeg::Tables) / 4); i += jpeg::kThreads) d[i] = s[i];
    }
    __syncthreads();
    const int zrl_len[2] = {(int)(T->ac[0][0xF0] >> 16), (int)(T->ac[1][0xF0] >> 16)};
    for (int f = blockIdx.x; f < p.n; f += gridDim.x) {
        const uint8_t* src = p.src + (size_t)f * p.H * row_bytes;
        uint8_t* dst = p.dst + (size_t)f * p.cap;
        for (int i = tid; i < jpeg::kHeaderBytes; i += jpeg::kThreads) dst[i] = T->header[i];      // (cap >= header + 2: the host refuses less)
        int out = jpeg::kHeaderBytes, carry_bits = 0, dcp0 = 0, dcp1 = 0, dcp2 = 0;
        uint32_t carry_byte = 0;
        for (int my = 0; my < g.mcu_rows; ++my) {
            jpeg::sample_stripe<jpeg::kThreads>(g, my, src, ws, ys, cs);   // (the raw rows alias the workspace)
            for (int t = tid; t < nb * 8; t += jpeg::kThreads) {          // DCT over the rows of every block
                const int b = t >> 3, r = t & 7, mx = b / jpeg::kBlocksPerMcu, k = b - mx * jpeg::kBlocksPerMcu;
                const uint8_t* sp = k < 4 ? ys + ((k >> 1) * 8 + r) * ystride + mx * 16 + (k & 1) * 8 : cs + ((k - 4) * 8 + r) * cstride + mx * 8;
                int d[8];
                for (int j = 0; j < 8; ++j) d[j] = (int)sp[j] - 128;
                jpeg::fdct_pass<true>(d);
                for (int j = 0; j < 8; ++j) ws[b * 64 + r * 8 + j] = (uint32_t)d[j];
            }
            __syncthreads();
            for (int t = tid; t < nb * 8; t += jpeg::kThreads) {          // ... over their columns, and the quantiser
                const int b = t >> 3, c = t & 7, mx = b / jpeg::kBlocksPerMcu, k = b - mx * jpeg::kBlocksPerMcu;
                int d[8];
                for (int r = 0; r < 8; ++r) d[r] = (int)ws[b * 64 + r * 8 + c];
                jpeg::fdct_pass<false>(d);
                const bool dummy = k < 4 && jpeg::y_dummy(g, my, mx, k);
                for (int r = 0; r < 8; ++r)
                    coef[b * jpeg::kCoefStride + T->zz_pos[r * 8 + c]] = dummy ? (int16_t)0 : (int16_t)jpeg::quantise(d[r], T->qv[k >= 4][r * 8 + c]);
            }
            __syncthreads();
            for (int i = tid; i < ws_dwords; i += jpeg::kThreads) ws[i] = i == 0 ? carry_byte << 24 : 0u;      // the bit stream starts with the partial byte so far
            if (tid < mw)                                                  // dummy blocks: the DC of the block before them in the MCU
                for (int k = 1; k < 4; ++k)
                    if (jpeg::y_dummy(g, my, tid, k)) coef[(tid * jpeg::kBlocksPerMcu + k) * jpeg::kCoefStride] = coef[(tid * jpeg::kBlocksPerMcu + k - 1) * jpeg::kCoefStride];
            __syncthreads();
            // one lane per block: its DC difference and code length
            int bits = 0, diff = 0, tbl = 0;
            const int16_t* cb = coef + min(tid, nb - 1) * jpeg::kCoefStride;
            if (tid < nb) {
                const int mx = tid / jpeg::kBlocksPerMcu, k = tid - mx * jpeg::kBlocksPerMcu;
                tbl = k >= 4;
                int pred;
                if (k >= 1 && k < 4) pred = cb[-jpeg::kCoefStride];
                else if (mx > 0) pred = coef[((mx - 1) * jpeg::kBlocksPerMcu + (k == 0 ? 3 : k)) * jpeg::kCoefStride];
                else pred = k == 0 ? dcp0 : k == 4 ? dcp1 : dcp2;
                diff = cb[0] - pred;
                const int s = jpeg::magnitude_bits(diff);
                bits = (int)(T->dc[tbl][s] >> 16) + s;
                int run = 0;
                for (int i = 1; i < 64; ++i) {
                    const int v = cb[i];
                    if (!v) { ++run; continue; }
                    bits += (run >> 4) * zrl_len[tbl];
                    const int sz = jpeg::magnitude_bits(v);
                    bits += (int)(T->ac[tbl][(run & 15) << 4 | sz] >> 16) + sz;
                    run = 0;
                }
                if (run) bits += (int)(T->ac[tbl][0] >> 16);
            }
            int total;
            const int start = carry_bits + block_scan(bits, scan, &total);
            if (tid < nb) {                                                // ... and its codes, ORed into the stream at its bit offset
                int w = start >> 5, fill = start & 31;
                unsigned long long acc = 0;
                auto put = [&](uint32_t code, int len) {                   // len in 1..16: fill stays below 48
                    acc |= (unsigned long long)code << (64 - fill - len);
                    fill += len;
                    if (fill >= 32) { atomicOr(&ws[w], (uint32_t)(acc >> 32)); acc <<= 32; fill -= 32; ++w; }
                };
                auto put_symbol = [&](uint32_t entry) { put(entry & 0xFFFFu, (int)(entry >> 16)); };
                const int s = jpeg::magnitude_bits(diff);
                put_symbol(T->dc[tbl][s]);
                if (s) put(jpeg::extra_bits(diff, s), s);
                int run = 0;
                for (int i = 1; i < 64; ++i) {
                    const int v = cb[i];
                    if (!v) { ++run; continue; }
                    for (; run > 15; run -= 16) put_symbol(T->ac[tbl][0xF0]);
                    const int sz = jpeg::magnitude_bits(v);
                    put_symbol(T->ac[tbl][run << 4 | sz]);
                    put(jpeg::extra_bits(v, sz), sz);
                    run = 0;
                }
                if (run) put_symbol(T->ac[tbl][0]);
                if (fill) atomicOr(&ws[w], (uint32_t)(acc >> 32));
            }
            __syncthreads();
            int stream_bits = carry_bits + total;
            if (my == g.mcu_rows - 1 && (stream_bits & 7)) {              // the end of the scan: 1-bits up to the byte boundary
                if (tid == 0) ws[stream_bits >> 5] |= (0xFFu >> (stream_bits & 7)) << (24 - 8 * ((stream_bits >> 3) & 3));
                stream_bits = (stream_bits + 7) & ~7;
                __syncthreads();
            }
            // whole bytes of the stream -> the slot, a zero byte behind every 0xFF; a thread takes a run of bytes
            const int nbytes = stream_bits >> 3;
            const int chunk = (((nbytes + jpeg::kThreads - 1) / jpeg::kThreads) + 3) & ~3;
            const int c0 = min(tid * chunk, nbytes), c1 = min(c0 + chunk, nbytes);
            int ff = 0;
            for (int j = c0; j < c1; ++j) ff += stream_byte(ws, j) == 255u;
            int total_ff;
            int pos = out + c0 + block_scan(ff, scan, &total_ff);
            for (int j = c0; j < c1; ++j) {                                // a file longer than the slot keeps counting and stops storing
                const uint32_t v = stream_byte(ws, j);
                if (pos < p.cap) dst[pos] = (uint8_t)v;
                ++pos;
                if (v == 255u) {
                    if (pos < p.cap) dst[pos] = 0;
                    ++pos;
                }
            }
            out += nbytes + total_ff;
            carry_bits = stream_bits & 7;
            carry_byte = carry_bits ? stream_byte(ws, nbytes) : 0u;       // (the bits behind the stream's end are zero)
            dcp0 = coef[((mw - 1) * jpeg::kBlocksPerMcu + 3) * jpeg::kCoefStride];
            dcp1 = coef[((mw - 1) * jpeg::kBlocksPerMcu + 4) * jpeg::kCoefStride];
            dcp2 = coef[((mw - 1) * jpeg::kBlocksPerMcu + 5) * jpeg::kCoefStride];
            __syncthreads();                                               // the next MCU row overwrites the stream and the blocks
        }
        if (tid == 0) {
            if (out < p.cap) dst[out] = 0xFF;
            if (out + 1 < p.cap) dst[out + 1] = 0xD9;
            const int total = out + 2;
            p.len[f] = total <= p.cap ? total : -total;
        }
    }
}

// the files that fit, back to back: off[i] = the sum of the fitting lengths before frame i (off[n]: of all), blob[off[i] ...] = slot i's file.
// A frame that did not fit (len < 0) takes no room.  Nothing is written at or beyond blob + blob_cap.  The lengths are filed behind off[n], so that one
// copy brings both to the host.
__global__ __launch_bounds__(256) void trs_jpeg_pack_kernel(const uint8_t* slots, const int32_t* len, int n, int cap, uint8_t* blob, long long blob_cap, long long* off)
{
    __shared__ long long part[4];
    const int tid = threadIdx.x;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        long long s = 0;
        for (int j = tid; j < f; j += 256) s += max(len[j], 0);
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
        __syncthreads();
        if ((tid & 63) == 0) part[tid >> 6] = s;
        __syncthreads();
        const long long base = part[0] + part[1] + part[2] + part[3];
        const int fit = max(len[f], 0);
        if (tid == 0) {
            off[f] = base;
            if (f == n - 1) off[n] = base + fit;
            reinterpret_cast<int32_t*>(off + n + 1)[f] = len[f];
        }
        const uint8_t* src = slots + (size_t)f * cap;
        for (int j = tid; j < fit; j += 256)
            if (base + j < blob_cap) blob[base + j] = src[j];
    }
}

int check_args(trs_env* e, int n_images, int quality, int cap)
{
    const int rc = jpeg::check_call(e, n_images, quality);
    if (rc) return rc;
    if (cap < jpeg::kHeaderBytes + 2) return trs_internal_fail(TRS_ERR_ARG, "cap is below the header's " + std::to_string(jpeg::kHeaderBytes) + " bytes plus the end marker's 2");
    return TRS_OK;
}

// the device copy of the tables for `quality`: rebuilt when the quality changes (the stream is drained first: a kernel in flight reads the old copy)
int ensure_tables(trs_env* e, int quality)
{
    if (e->jpg_quality == quality && e->jpg_tab.get()) return TRS_OK;
    std::unique_ptr<jpeg::Tables> t(new jpeg::Tables);
    std::memset(t.get(), 0, sizeof(jpeg::Tables));
    jpeg::build_tables(e->H, e->W, quality, t.get());
    HIPCHK(hipStreamSynchronize(e->sP));
    e->jpg_quality = 0;
    HIPCHK(e->jpg_tab.reserve(sizeof(jpeg::Tables)));
    HIPCHK(hipMemcpy(e->jpg_tab.get(), t.get(), sizeof(jpeg::Tables), hipMemcpyHostToDevice));
    trs_internal_count(e, 0, sizeof(jpeg::Tables));
    e->jpg_quality = quality;
    return TRS_OK;
}
}  // namespace

TRS_EXPORT int trs_jpeg_header_bytes(trs_env* e, int quality)
{
    const int rc = jpeg::check_call(e, 1, quality);       // (the header's length does not depend on the number of images)
    return rc ? rc : jpeg::kHeaderBytes;
}

TRS_EXPORT int trs_encode_jpeg(trs_env* e, const uint8_t* d_src, int n_images, int quality, uint8_t* d_dst, int cap, int32_t* d_len)
{
    int rc = check_args(e, n_images, quality, cap);
    if (rc) return rc;
    if (!d_dst || !d_len) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    if (reinterpret_cast<uintptr_t>(d_src) & 3) return trs_internal_fail(TRS_ERR_ARG, "d_src must be 4-byte aligned");
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    rc = jpeg::latest_frame_source(e, n_images, "to encode", &d_src);
    if (rc) return rc;
    const jpeg::Geometry g = jpeg::geometry(e->H, e->W);
    const jpeg::StripeLds lds = jpeg::stripe_lds(e->W);
    if (jpeg::blocks_per_stripe(g) > jpeg::kThreads || lds.total > jpeg::kMaxLdsBytes || e->H > 65535 || e->W > 65535)
        return trs_internal_fail(TRS_ERR_LIMIT, "image too wide for the encoder: a lane per block of an MCU row allows img_w <= " + std::to_string(jpeg::kThreads / jpeg::kBlocksPerMcu * 16));
    rc = ensure_tables(e, quality);
    if (rc) return rc;
    JpegParams p{};
    p.src = d_src; p.dst = d_dst; p.len = d_len; p.tab = reinterpret_cast<const jpeg::Tables*>(e->jpg_tab.get());
    p.n = n_images; p.H = e->H; p.W = e->W; p.cap = cap; p.lds = lds;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_jpeg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds.total));
    const int grid = std::min(n_images, std::max(1, e->cu_count) * jpeg::kWgsPerCu);
    hipLaunchKernelGGL(trs_jpeg_kernel, dim3(grid), dim3(jpeg::kThreads), lds.total, e->sP, p);
    HIPCHK(hipGetLastError());
    trsim::resident_note_launch(e);                       // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return TRS_OK;
}

TRS_EXPORT int trs_encode_jpeg_host(trs_env* e, const uint8_t* d_src, int n_images, int quality, int cap, uint8_t* h_blob, size_t blob_cap, int64_t* h_off, int32_t* h_len)
{
    int rc = check_args(e, n_images, quality, cap);
    if (rc) return rc;
    if (!h_off || (!h_blob && blob_cap)) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    HIPCHK(hipSetDevice(e->device));
    const size_t n = (size_t)n_images, slot_bytes = n * (size_t)cap, off_bytes = (n + 1) * sizeof(long long), pin_bytes = off_bytes + n * sizeof(int32_t);
    if (e->jpg_slots.bytes() < slot_bytes || e->jpg_len.bytes() < n * sizeof(int32_t) || e->jpg_pin.bytes() < pin_bytes) {
        rc = trsim::quiesce_handle(e);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(e->sP));                              // what is replaced may still be in use
        hipError_t rh = e->jpg_slots.reserve(slot_bytes);
        if (rh == hipSuccess) rh = e->jpg_blob.reserve(slot_bytes);
        if (rh == hipSuccess) rh = e->jpg_len.reserve(n * sizeof(int32_t));
        if (rh == hipSuccess) rh = e->jpg_off.reserve(pin_bytes);
        if (rh == hipSuccess) rh = e->jpg_pin.reserve(pin_bytes);
        if (rh != hipSuccess) return jpeg::no_memory(rh, 2 * slot_bytes, "encoder scratch");
    }
    rc = trs_encode_jpeg(e, d_src, n_images, quality, e->jpg_slots.get(), cap, e->jpg_len.get());
    if (rc) return rc;
    const size_t copy_bytes = std::min(blob_cap, slot_bytes);
    const int grid = std::min(n_images, std::max(1, e->cu_count) * 4);
    hipLaunchKernelGGL(trs_jpeg_pack_kernel, dim3(grid), dim3(256), 0, e->sP, e->jpg_slots.get(), e->jpg_len.get(), n_images, cap, e->jpg_blob.get(),
                       (long long)copy_bytes, e->jpg_off.get());
    HIPCHK(hipGetLastError());
    unsigned char* pin = e->jpg_pin.get();
    HIPCHK(hipMemcpyAsync(pin, e->jpg_off.get(), pin_bytes, hipMemcpyDeviceToHost, e->sP));                       // offsets | lengths
    if (copy_bytes) HIPCHK(hipMemcpyAsync(h_blob, e->jpg_blob.get(), copy_bytes, hipMemcpyDeviceToHost, e->sP));   // (the files' total is not known before the one synchronisation)
    HIPCHK(hipStreamSynchronize(e->sP));
    trs_internal_count(e, pin_bytes + copy_bytes, 0);
    std::memcpy(h_off, pin, off_bytes);
    if (h_len) std::memcpy(h_len, pin + off_bytes, n * sizeof(int32_t));
    if ((unsigned long long)h_off[n] > blob_cap)
        return trs_internal_fail(TRS_ERR_LIMIT, "the files take " + std::to_string(h_off[n]) + " bytes, blob_cap is " + std::to_string(blob_cap));
    return TRS_OK;
}
