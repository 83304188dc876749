// trsim_jpeg_codec.hip — the camera codec: uint8[n][H][W][3] frames on the device -> the frames a JPEG save and open would give back, byte for byte
// what include/trsim_spec.h ("camera codec (JPEG round trip)") defines: decode(encode(frame, q)) without a file in between.  Every rule comes from
// trsim_jpeg_tables.hpp and trsim_jpeg_decode.hpp through the block steps of trsim_jpeg_codec.hpp, the first and the last stage from trsim_jpeg_device.hpp
// (shared with the encoder and with the decoder); this file holds the data movement of trs_jpeg_codec_kernel between them, the entry points, and the
// pre-pass trs_step_pilot runs while trs_set_camera_codec is set.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_jpeg_codec.hpp"
#include "trsim_jpeg_device.hpp"
#include "trsim_jpeg_host.hpp"

namespace {
namespace jpeg = trsim::jpeg;
using jpeg::wave_sync;

struct CodecParams {
    const uint8_t* src;          // uint8[n][H][W][3], 4-byte aligned, W % 4 == 0
    uint8_t* dst;                // the same shape, no byte shared with src
    const int32_t* qv;           // quant_steps: int32[2][64]
    int n, H, W;
    jpeg::CodecLds lds;
};

extern __shared__ __attribute__((aligned(16))) unsigned char csmem[];

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
    const jpeg::SampleBuffers sb{csmem + p.lds.off_yout, csmem + p.lds.off_cring, mw};
    const int ystride = 16 * mw, cstride = 8 * mw, row_bytes = p.W * 3, j = lane & 7;
    if (tid < 128) Q[tid] = p.qv[tid];
    for (int f = blockIdx.x; f < p.n; f += gridDim.x) {
        const uint8_t* src = p.src + (size_t)f * p.H * row_bytes;
        uint8_t* dst = p.dst + (size_t)f * p.H * row_bytes;
        for (int my = 0; my < g.mcu_rows; ++my) {
            jpeg::sample_stripe<jpeg::kCodecThreads>(g, my, src, raw4, ys, cs);
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
                    sb.store_block_row(my, mx, k, j, lo4, hi4);
                }
                wave_sync();                                                                  // the wave's intermediates are free for its next 8 blocks
            }
            __syncthreads();
            if (my > 0) jpeg::output_mcu_row<jpeg::kCodecThreads>(g, my - 1, sb, dst, tid, true);   // (dwords: the host refuses a d_dst that is not 4-byte aligned, and img_w % 4 == 0)
            // (what the next MCU row overwrites of the samples read here lies behind its two barriers)
        }
        jpeg::output_mcu_row<jpeg::kCodecThreads>(g, g.mcu_rows - 1, sb, dst, tid, true);
    }
}

// the device copy of quant_steps(quality): rebuilt when the quality changes (the stream is drained first: a kernel in flight reads the old copy)
int ensure_steps(trs_env* e, int quality)
{
    if (e->jpc_quality == quality && e->jpc_steps.get()) return TRS_OK;
    int32_t qv[2][64];
    jpeg::quant_steps(quality, qv);
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
}  // namespace

TRS_EXPORT int trs_jpeg_roundtrip(trs_env* e, const uint8_t* d_src, int n_images, int quality, uint8_t* d_dst, const uint8_t** d_out)
{
    int rc = jpeg::check_call(e, n_images, quality);
    if (rc) return rc;
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 3) return trs_internal_fail(TRS_ERR_ARG, "d_src and d_dst must be 4-byte aligned");
    rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    rc = jpeg::latest_frame_source(e, n_images, "for the codec", &d_src);
    if (rc) return rc;
    const size_t frame_bytes = (size_t)e->H * e->W * 3, bytes = (size_t)n_images * frame_bytes;
    if (!d_dst) {
        if (n_images > e->n) return trs_internal_fail(TRS_ERR_ARG, "own buffer holds n_envs frames");
        const hipError_t rh = e->jpc_dst.reserve((size_t)e->n * frame_bytes);      // (allocated once: the size is fixed)
        if (rh != hipSuccess) return jpeg::no_memory(rh, (size_t)e->n * frame_bytes, "camera codec frames");
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
    int rc = jpeg::check_call(e, n_images, quality);
    if (rc) return rc;
    if (!h_dst) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    const size_t bytes = (size_t)n_images * e->H * e->W * 3;
    if (e->jpc_in.bytes() < (h_src ? bytes : 0) || e->jpc_out.bytes() < bytes) {
        HIPCHK(hipStreamSynchronize(e->sP));                              // what is replaced may still be in use
        hipError_t rh = h_src ? e->jpc_in.reserve(bytes) : hipSuccess;
        if (rh == hipSuccess) rh = e->jpc_out.reserve(bytes);
        if (rh != hipSuccess) return jpeg::no_memory(rh, 2 * bytes, "camera codec frames");
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
    if (e->scene.has_filter)
        return trs_internal_fail(TRS_ERR_STATE, "a frame filter is set (trs_set_frame_filter): it would run in front of the codec, the reference filters the decoded frame: "
                                                "remove it and run trs_preprocess on the codec's frames");
    int rc = check_size(e);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    const size_t bytes = (size_t)e->n * e->H * e->W * 3;
    const hipError_t rh = e->jpc_dst.reserve(bytes);
    if (rh != hipSuccess) return jpeg::no_memory(rh, bytes, "camera codec frames");
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
