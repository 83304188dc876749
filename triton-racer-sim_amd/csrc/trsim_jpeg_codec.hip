// trsim_jpeg_codec.hip — the camera codec: uint8[n][H][W][3] frames on the device -> the frames a JPEG save and open would give back, byte for byte
// what include/trsim_spec.h ("camera codec (JPEG round trip)") defines: decode(encode(frame, q)) without a file in between.  Every rule comes from
// trsim_jpeg_tables.hpp and trsim_jpeg_decode.hpp through the block steps of trsim_jpeg_codec.hpp; this file holds the data movement of
// trs_jpeg_codec_kernel, the entry points, and the pre-pass trs_step_pilot runs while trs_set_camera_codec is set.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_jpeg_codec.hpp"

namespace {
namespace jpeg = trsim::jpeg;

struct CodecParams {
    const uint8_t* src;          // uint8[n][H][W][3], 4-byte aligned, W % 4 == 0
    uint8_t* dst;                // the same shape, no byte shared with src
    const int32_t* qv;           // codec_steps: int32[2][64]
    int n, H, W;
    jpeg::CodecLds lds;
};

extern __shared__ __attribute__((aligned(16))) unsigned char csmem[];

// what one lane of the wave wrote to LDS is visible to the others behind this
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// image rows [16 my, 16 my + 16) of the frame from the Y samples of MCU row my and the chroma ring: 4 pixels (3 dwords) per thread and turn
__device__ void output_mcu_row(const CodecParams& p, const jpeg::Geometry& g, int my, const uint8_t* yout, const uint8_t* cring, uint8_t* dst)
{
    const int mw = g.mcu_cols, ys = 16 * mw, cs = 8 * mw, units = p.W >> 2, rows = min(16, p.H - 16 * my);
    const uint8_t* yrow0 = yout + (my & 1) * 256 * mw;
    auto crow = [&](int plane, int r) { return cring + ((r >> 3) % jpeg::kChromaRing) * 128 * mw + plane * 64 * mw + (r & 7) * cs; };
    for (int t = threadIdx.x; t < rows * units; t += jpeg::kCodecThreads) {
        const int ry = t / units, u = t - ry * units, y = 16 * my + ry, x0 = 4 * u;
        const int r0 = y >> 1, r1 = jpeg::chroma_nb_row(g, y);
        // the vertical sums of the chroma columns 2u - 1 .. 2u + 2 (clamped to the plane), both planes
        int s[2][4];
        for (int pl = 0; pl < 2; ++pl) {
            const uint8_t* a = crow(pl, r0);
            const uint8_t* b = crow(pl, r1);
            for (int j = 0; j < 4; ++j) {
                const int c = min(max(2 * u - 1 + j, 0), jpeg::chroma_cols(p.W) - 1);
                s[pl][j] = jpeg::tri_v(a[c], b[c]);
            }
        }
        const uint32_t y4 = *reinterpret_cast<const uint32_t*>(yrow0 + ry * ys + x0);
        uint32_t px[4];
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + k, own = 1 + (k >> 1), nb = (k & 1) ? own + 1 : own - 1;      // (s[][0] and s[][3] are the clamped neighbours)
            px[k] = jpeg::ycc_to_rgb((int)((y4 >> (8 * k)) & 255u), jpeg::tri_h(s[0][own], s[0][nb], x), jpeg::tri_h(s[1][own], s[1][nb], x));
        }
        uint32_t* o4 = reinterpret_cast<uint32_t*>(dst + ((size_t)y * p.W + x0) * 3);
        o4[0] = px[0] | px[1] << 24;
        o4[1] = px[1] >> 8 | px[2] << 16;
        o4[2] = px[2] >> 16 | px[3] << 8;
    }
}

// One workgroup per frame at a time, one MCU row (16 image rows) at a time:
//   raw RGB rows -> LDS | colour + 2x2 downsampling -> sample planes | per wave, 8 blocks at a time: rows in, columns (quantiser and dequantiser), rows out
//   -> the Y samples of this MCU row and its slot of the chroma ring | the image rows of the MCU row BEFORE this one -> the frame (the triangle filter
//   reads the first chroma row of this one, and the last of the one before that).
// Dummy Y blocks are skipped: no image pixel lies in them.  The chroma planes' padding rows and columns are transformed with their blocks and not read after.
__global__ __launch_bounds__(jpeg::kCodecThreads) void trs_jpeg_codec_kernel(CodecParams p)
{
    const jpeg::Geometry g = jpeg::geometry(p.H, p.W);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mw = g.mcu_cols, nb = jpeg::blocks_per_stripe(g);
    int32_t* Q = reinterpret_cast<int32_t*>(csmem + p.lds.off_q);
    uint32_t* raw4 = reinterpret_cast<uint32_t*>(csmem + p.lds.off_raw);   // the stripe's image rows, as they lie in memory
    uint8_t* ys = csmem + p.lds.off_y;                                      // [16][16 mw]
    uint8_t* cs = csmem + p.lds.off_c;                                      // [2][8][8 mw]
    int32_t* w = reinterpret_cast<int32_t*>(csmem + p.lds.off_ws) + (wave * 8 + (lane >> 3)) * jpeg::kWsBlockStride;   // this lane's block of the wave's 8
    uint8_t* yout = csmem + p.lds.off_yout;                                 // [2][16][16 mw]
    uint8_t* cring = csmem + p.lds.off_cring;                               // [kChromaRing][Cb | Cr][8][8 mw]
    const int ystride = 16 * mw, cstride = 8 * mw, row_bytes = p.W * 3, row_dw = row_bytes / 4, j = lane & 7;
    if (tid < 128) Q[tid] = p.qv[tid];
    for (int f = blockIdx.x; f < p.n; f += gridDim.x) {
        const uint8_t* src = p.src + (size_t)f * p.H * row_bytes;
        uint8_t* dst = p.dst + (size_t)f * p.H * row_bytes;
        for (int my = 0; my < g.mcu_rows; ++my) {
            const int r_lo = 16 * my, nrows = min(16, p.H - r_lo);
            {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + (size_t)r_lo * row_bytes);
                for (int i = tid; i < nrows * row_dw; i += jpeg::kCodecThreads) raw4[i] = s4[i];
            }
            __syncthreads();
            {   // colour and downsampling, one 2 x 2 quad of the padded planes per thread and turn
                const uint8_t* raw = reinterpret_cast<const uint8_t*>(raw4);
                for (int q = tid; q < 8 * cstride; q += jpeg::kCodecThreads) {
                    const int qr = q / cstride, qc = q - qr * cstride;
                    for (int dy = 0; dy < 2; ++dy)
                        for (int dx = 0; dx < 2; ++dx) {
                            const uint8_t* px = raw + (jpeg::y_src_row(g, r_lo + 2 * qr + dy) - r_lo) * row_bytes + jpeg::y_src_col(g, 2 * qc + dx) * 3;
                            ys[(2 * qr + dy) * ystride + 2 * qc + dx] = (uint8_t)jpeg::luma(px[0], px[1], px[2]);
                        }
                    int r0, r1, c0, c1;
                    jpeg::c_src_rows(g, 8 * my + qr, &r0, &r1);
                    jpeg::c_src_cols(g, qc, &c0, &c1);
                    const uint8_t* a = raw + (r0 - r_lo) * row_bytes + c0 * 3;
                    const uint8_t* b = raw + (r0 - r_lo) * row_bytes + c1 * 3;
                    const uint8_t* c = raw + (r1 - r_lo) * row_bytes + c0 * 3;
                    const uint8_t* d = raw + (r1 - r_lo) * row_bytes + c1 * 3;
                    cs[qr * cstride + qc] = (uint8_t)jpeg::downsample(jpeg::chroma_b(a[0], a[1], a[2]), jpeg::chroma_b(b[0], b[1], b[2]),
                                                                      jpeg::chroma_b(c[0], c[1], c[2]), jpeg::chroma_b(d[0], d[1], d[2]), qc);
                    cs[(8 + qr) * cstride + qc] = (uint8_t)jpeg::downsample(jpeg::chroma_r(a[0], a[1], a[2]), jpeg::chroma_r(b[0], b[1], b[2]),
                                                                            jpeg::chroma_r(c[0], c[1], c[2]), jpeg::chroma_r(d[0], d[1], d[2]), qc);
                }
            }
            __syncthreads();
            for (int b0 = wave * 8; b0 < nb; b0 += (jpeg::kCodecThreads / 64) * 8) {      // 8 blocks per wave and turn: a row, a column, a row per lane
                const int b = b0 + (lane >> 3), mx = b / jpeg::kBlocksPerMcu, k = b - mx * jpeg::kBlocksPerMcu;
                const bool live = b < nb && !(k < 4 && jpeg::y_dummy(g, my, mx, k));
                int32_t d[8];
                if (live) {
                    const uint8_t* sp = k < 4 ? ys + ((k >> 1) * 8 + j) * ystride + mx * 16 + (k & 1) * 8 : cs + ((k - 4) * 8 + j) * cstride + mx * 8;
                    const uint32_t lo4 = reinterpret_cast<const uint32_t*>(sp)[0], hi4 = reinterpret_cast<const uint32_t*>(sp)[1];
                    for (int c = 0; c < 4; ++c) {
                        d[c] = (int32_t)((lo4 >> (8 * c)) & 255u);
                        d[c + 4] = (int32_t)((hi4 >> (8 * c)) & 255u);
                    }
                    jpeg::codec_row_in(d);
                    for (int c = 0; c < 8; ++c) w[j * jpeg::kWsRowStride + c] = d[c];
                }
                wave_sync();
                if (live) {
                    for (int r = 0; r < 8; ++r) d[r] = w[r * jpeg::kWsRowStride + j];
                    jpeg::codec_column(d, Q + (k >= 4 ? 64 : 0), j);
                    for (int r = 0; r < 8; ++r) w[r * jpeg::kWsRowStride + j] = d[r];
                }
                wave_sync();
                if (live) {
                    for (int c = 0; c < 8; ++c) d[c] = w[j * jpeg::kWsRowStride + c];
                    jpeg::codec_row_out(d);
                    uint32_t lo4 = 0, hi4 = 0;
                    for (int c = 0; c < 4; ++c) {
                        lo4 |= (uint32_t)d[c] << (8 * c);
                        hi4 |= (uint32_t)d[c + 4] << (8 * c);
                    }
                    uint8_t* out = k < 4 ? yout + (my & 1) * 256 * mw + (8 * (k >> 1) + j) * ystride + 16 * mx + 8 * (k & 1)
                                         : cring + (my % jpeg::kChromaRing) * 128 * mw + (k - 4) * 64 * mw + j * cstride + 8 * mx;
                    reinterpret_cast<uint32_t*>(out)[0] = lo4;
                    reinterpret_cast<uint32_t*>(out)[1] = hi4;
                }
                wave_sync();                                                                  // the wave's intermediates are free for its next 8 blocks
            }
            __syncthreads();
            if (my > 0) output_mcu_row(p, g, my - 1, yout, cring, dst);
            // (what the next MCU row overwrites of the samples read here lies behind its two barriers)
        }
        output_mcu_row(p, g, g.mcu_rows - 1, yout, cring, dst);
    }
}

// the device copy of codec_steps(quality): rebuilt when the quality changes (the stream is drained first: a kernel in flight reads the old copy)
int ensure_steps(trs_env* e, int quality)
{
    if (e->jpc_quality == quality && e->jpc_steps.get()) return TRS_OK;
    int32_t qv[128];
    jpeg::codec_steps(quality, qv);
    HIPCHK(hipStreamSynchronize(e->sP));
    e->jpc_quality = 0;
    HIPCHK(e->jpc_steps.reserve(sizeof qv));
    HIPCHK(hipMemcpy(e->jpc_steps.get(), qv, sizeof qv, hipMemcpyHostToDevice));
    trs_internal_count(e, 0, sizeof qv);
    e->jpc_quality = quality;
    return TRS_OK;
}

// what every entry point refuses about the handle's image size (TRS_OK otherwise)
int check_size(const trs_env* e)
{
    if (!jpeg::codec_size_ok(e->H, e->W))
        return trs_internal_fail(TRS_ERR_LIMIT, "image too narrow for the camera codec: the triangle filter needs a chroma plane of more than two columns, img_w > 4");
    if (jpeg::codec_lds(e->W).total > jpeg::kMaxLdsBytes)
        return trs_internal_fail(TRS_ERR_LIMIT, "image too wide for the camera codec: a 16-row stripe with its sample planes in " + std::to_string(jpeg::kMaxLdsBytes) +
                                                    " bytes of LDS allows img_w <= " + std::to_string(jpeg::codec_max_width(jpeg::kMaxLdsBytes)));
    return TRS_OK;
}

int no_memory(hipError_t rh, size_t bytes)
{
    return trs_internal_fail(rh == hipErrorOutOfMemory ? TRS_ERR_NOMEM : TRS_ERR_DEVICE, "no memory for " + std::to_string(bytes) + " bytes of camera codec frames");
}
}  // namespace

TRS_EXPORT int trs_jpeg_roundtrip(trs_env* e, const uint8_t* d_src, int n_images, int quality, uint8_t* d_dst, const uint8_t** d_out)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (quality < 1 || quality > 100) return trs_internal_fail(TRS_ERR_ARG, "quality must be in [1, 100]");
    if (n_images < 1) return trs_internal_fail(TRS_ERR_ARG, "n_images < 1");
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3) return trs_internal_fail(TRS_ERR_ARG, "d_src and d_dst must be 4-byte aligned");
    int rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    if (!d_src) {
        d_src = trs_internal_latest_frame(e);
        if (!d_src) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0): there is no latest frame for the codec");
        if (n_images != e->n) return trs_internal_fail(TRS_ERR_ARG, "latest-frame source needs n_images == n_envs");
    }
    const size_t frame_bytes = (size_t)e->H * e->W * 3, bytes = (size_t)n_images * frame_bytes;
    if (!d_dst) {
        if (n_images > e->n) return trs_internal_fail(TRS_ERR_ARG, "own buffer holds n_envs frames");
        const hipError_t rh = e->jpc_dst.reserve((size_t)e->n * frame_bytes);      // (allocated once: the size is fixed)
        if (rh != hipSuccess) return no_memory(rh, (size_t)e->n * frame_bytes);
        d_dst = e->jpc_dst.get();
    }
    if (d_dst < d_src + bytes && d_src < d_dst + bytes)
        return trs_internal_fail(TRS_ERR_ARG, "d_dst overlaps d_src: a pixel is made from its neighbours' blocks, the codec does not work in place");
    rc = ensure_steps(e, quality);
    if (rc) return rc;
    if (d_out) *d_out = d_dst;
    CodecParams p{};
    p.src = d_src; p.dst = d_dst; p.qv = e->jpc_steps.get();
    p.n = n_images; p.H = e->H; p.W = e->W; p.lds = jpeg::codec_lds(e->W);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_jpeg_codec_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, p.lds.total));
    const int grid = std::min(n_images, std::max(1, e->cu_count) * jpeg::kCodecWgsPerCu);
    hipLaunchKernelGGL(trs_jpeg_codec_kernel, dim3(grid), dim3(jpeg::kCodecThreads), p.lds.total, e->sP, p);
    HIPCHK(hipGetLastError());
    trsim::resident_note_launch(e);                       // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return TRS_OK;
}

TRS_EXPORT int trs_jpeg_roundtrip_host(trs_env* e, const uint8_t* h_src, int n_images, int quality, uint8_t* h_dst)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (quality < 1 || quality > 100) return trs_internal_fail(TRS_ERR_ARG, "quality must be in [1, 100]");
    if (n_images < 1) return trs_internal_fail(TRS_ERR_ARG, "n_images < 1");
    if (!h_dst) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    int rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    const size_t bytes = (size_t)n_images * e->H * e->W * 3;
    if (e->jpc_in.bytes() < (h_src ? bytes : 0) || e->jpc_out.bytes() < bytes) {
        HIPCHK(hipStreamSynchronize(e->sP));                              // what is replaced may still be in use
        hipError_t rh = h_src ? e->jpc_in.reserve(bytes) : hipSuccess;
        if (rh == hipSuccess) rh = e->jpc_out.reserve(bytes);
        if (rh != hipSuccess) return no_memory(rh, 2 * bytes);
    }
    if (h_src) HIPCHK(hipMemcpyAsync(e->jpc_in.get(), h_src, bytes, hipMemcpyHostToDevice, e->sP));
    rc = trs_jpeg_roundtrip(e, h_src ? e->jpc_in.get() : nullptr, n_images, quality, e->jpc_out.get(), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h_dst, e->jpc_out.get(), bytes, hipMemcpyDeviceToHost, e->sP));
    HIPCHK(hipStreamSynchronize(e->sP));
    trs_internal_count(e, bytes, h_src ? bytes : 0);
    return TRS_OK;
}

TRS_EXPORT int trs_set_camera_codec(trs_env* e, int quality)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (quality < 0 || quality > 100) return trs_internal_fail(TRS_ERR_ARG, "quality must be in [1, 100], or 0 for no codec");
    if (quality == 0) { e->codec_quality = 0; return TRS_OK; }
    if (!e->cfg.render) return trs_internal_fail(TRS_ERR_STATE, "the env has no camera (cfg.render == 0)");
    if (e->has_frame_filter)
        return trs_internal_fail(TRS_ERR_STATE, "a frame filter is set (trs_set_frame_filter): it would run in front of the codec, the reference filters the decoded frame: "
                                                "remove it and run trs_preprocess on the codec's frames");
    int rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    const size_t bytes = (size_t)e->n * e->H * e->W * 3;
    const hipError_t rh = e->jpc_dst.reserve(bytes);
    if (rh != hipSuccess) return no_memory(rh, bytes);
    rc = ensure_steps(e, quality);
    if (rc) return rc;
    e->codec_quality = quality;
    return TRS_OK;
}

TRS_EXPORT int trs_get_camera_codec(trs_env* e, int* quality)
{
    if (!e || !quality) return trs_internal_fail(TRS_ERR_ARG, "null handle or destination");
    *quality = e->codec_quality;
    return TRS_OK;
}

// trs_step_pilot's pre-pass while a camera codec is set: codec(frames) of the n_envs frames the pilot reads today, in the handle's codec buffer
int trs_internal_camera_codec(trs_env* e, const uint8_t* d_frames, const uint8_t** d_out)
{
    return trs_jpeg_roundtrip(e, d_frames, e->n, e->codec_quality, nullptr, d_out);
}
