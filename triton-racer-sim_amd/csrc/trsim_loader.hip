// trsim_loader.hip — the training minibatches of libtrsim.so (include/trsim_spec.h, "training minibatches"): DataLoader.load's split, shuffle and batch
// (components/keras_train.py:33-69) over a set that stays uint8 on the device.  One kernel, trs_batch_kernel, gathers the records of one minibatch:
// frames normalised into the layout and type the training step wants, features, labels and record numbers.  The rules (refusals, permutation, split
// offsets, row -> features / labels) are trsim_loader.hpp, shared with trs_loader_order, which gives the same order on the host without a GPU.
//
// Work is cut into (batch slot, chunk of the frame) items of kUnitsPerItem units; the grid is sized from the CU count and strides over the items.  An
// item's record number depends on the workgroup's index alone, so it is wave-uniform: the Feistel rounds and the cycle walk run once per wave on the
// scalar unit and cannot diverge.  Lanes take CONSECUTIVE units, so every load and store instruction of a wave covers one contiguous run:
//   NHWC  unit = one dword of the frame (4 bytes)         -> one 16-B (float32) or 8-B (binary16) store; 1 KiB per float32 store instruction
//   NHWC  uint8: a copy, unit = four dwords               -> one 16-B load and one 16-B store, the frame's last 0..3 dwords one by one
//   NCHW  unit = four pixels (three dwords, one load)     -> one 16-B or 8-B store into each of the three planes
// A frame starts at a multiple of H * W * 3 bytes, which W % 4 == 0 makes a multiple of 4 and no more (a 3 x 4 frame has 36 bytes): the wide loads (and
// the uint8 copy's stores) are typed as 4-byte aligned and the compiler emits what the target allows for that; nothing assumes more.  A slot's float32
// images start at a multiple of 16 bytes from the 16-byte aligned base and its binary16 images at a multiple of 8, the widths of their stores.
// No LDS, no atomics.  The features, labels and record number of a slot are written by lane 0 of the slot's first item.  Bound: HBM — a float32 batch
// reads R bytes and writes 4 R.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_batch.hpp"
#include "trsim_loader.hpp"

namespace {

using namespace trsim;                 // trsim_batch.hpp: BatchParams, the 4-byte-aligned wide types, store4

template <int LAYOUT, int DTYPE>
__global__ __launch_bounds__(kBatchBlock) void trs_batch_kernel(const BatchParams p)
{
    for (uint32_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint32_t slot = item / p.chunks, chunk = item - slot * p.chunks;
        const uint32_t rec = p.order.record(p.first + slot);                 // wave-uniform
        if (chunk == 0 && threadIdx.x == 0) {
            const trsim::Sample s = trsim::row_to_sample(p.rows + (size_t)rec * trsim::kLoaderRowFloats, p.loader, p.label);
            for (int f = 0; f < p.n_feat; ++f) p.features[(size_t)slot * p.n_feat + f] = s.feat[f];
            p.labels[(size_t)slot * 2] = s.label[0]; p.labels[(size_t)slot * 2 + 1] = s.label[1];
            if (p.index) p.index[slot] = (int32_t)rec;
        }
        if (!p.frames) continue;
        const uint32_t* src = p.frames + (size_t)rec * p.frame_dwords;
#pragma unroll
        for (int k = 0; k < kBatchUnroll; ++k) {
            const uint32_t u = chunk * kUnitsPerItem + k * kBatchBlock + threadIdx.x;
            if (u >= p.units) continue;
            if (LAYOUT == TRS_LAYOUT_NHWC && DTYPE == TRS_DTYPE_U8) {                        // a plain copy: 16 bytes per lane, the frame's last 0..3 dwords one by one
                uint32_t* dst = static_cast<uint32_t*>(p.images) + (size_t)slot * p.frame_dwords;
                if (4 * u + 3 < p.frame_dwords) *reinterpret_cast<dwords4_a4*>(dst + 4 * (size_t)u) = *reinterpret_cast<const dwords4_a4*>(src + 4 * (size_t)u);
                else for (uint32_t d = 4 * u; d < p.frame_dwords; ++d) dst[d] = src[d];
            } else if (LAYOUT == TRS_LAYOUT_NHWC) {
                const uint32_t w = src[u];
                store4<DTYPE>(p.images, (size_t)slot * p.frame_dwords + u, byte_of(w, 0), byte_of(w, 1), byte_of(w, 2), byte_of(w, 3));
            } else {
                const dwords3_a4 w = *reinterpret_cast<const dwords3_a4*>(src + 3 * (size_t)u);
                const uint32_t w0 = w.x, w1 = w.y, w2 = w.z;                          // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
                const size_t e = (size_t)slot * 3 * p.quads + u;
                store4<DTYPE>(p.images, e, byte_of(w0, 0), byte_of(w0, 3), byte_of(w1, 2), byte_of(w2, 1));
                store4<DTYPE>(p.images, e + p.quads, byte_of(w0, 1), byte_of(w1, 0), byte_of(w1, 3), byte_of(w2, 2));
                store4<DTYPE>(p.images, e + 2 * (size_t)p.quads, byte_of(w0, 2), byte_of(w1, 1), byte_of(w2, 0), byte_of(w2, 3));
            }
        }
    }
}

template <int LAYOUT, int DTYPE>
void launch_batch(const trs_env* e, const BatchParams& p, int grid)
{
    hipLaunchKernelGGL((trs_batch_kernel<LAYOUT, DTYPE>), dim3(grid), dim3(kBatchBlock), 0, e->sP, p);
}

}  // namespace

TRS_EXPORT void trs_default_loader_config(trs_loader_config* cfg)
{
    if (cfg) trsim::loader_defaults(cfg);
}

TRS_EXPORT int trs_loader_order(const trs_loader_config* cfg, int split, int epoch, int first, int count, int32_t* h_index)
{
    if (const char* why = trsim::loader_config_error(cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (const char* why = trsim::loader_range_error(cfg, split, epoch, first, count)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (count > 0 && !h_index) return trs_internal_fail(TRS_ERR_ARG, "h_index is NULL");
    const trsim::Order o = trsim::Order::of(cfg->seed, cfg->n_records, cfg->n_train, split, epoch);
    for (int k = 0; k < count; ++k) h_index[k] = (int32_t)o.record((uint32_t)(first + k));
    return TRS_OK;
}

// The one path of trs_sample_batch and trs_sample_batch_aug: the refusals, the work items, one launch.  No augmentation (aug == nullptr or everything
// off) launches trs_batch_kernel; otherwise trs_batch_aug_kernel (trsim_augment.hip), whose unit is four pixels in every layout.
int trsim::sample_batch(trs_env* e, const trs_loader_config* cfg, const trs_augment_config* aug, const uint8_t* d_frames, const float* d_rows, int split,
                        int epoch, int first, int batch, void* d_images, float* d_features, float* d_labels, int32_t* d_index)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (const char* why = trsim::loader_config_error(cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (const char* why = trsim::loader_range_error(cfg, split, epoch, first, batch)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (aug) if (const char* why = trsim::augment_config_error(aug, cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    const trsim::LoaderCall call{d_frames, d_rows, d_images, d_features, d_labels, d_index, e->cfg.render != 0};
    if (const char* why = trsim::loader_call_error(cfg, call)) return trs_internal_fail(TRS_ERR_ARG, why);
    HIPCHK(hipSetDevice(e->device));
    if (batch == 0) return TRS_OK;
    { int rq = trsim::quiesce_handle(e); if (rq) return rq; }
    const bool plain = trsim::augment_is_off(aug);
    BatchParams p{};
    p.frames = reinterpret_cast<const uint32_t*>(d_frames); p.rows = d_rows;
    p.images = d_images; p.features = d_features; p.labels = d_labels; p.index = d_index;
    p.order = trsim::Order::of(cfg->seed, cfg->n_records, cfg->n_train, split, epoch);
    p.first = (uint32_t)first; p.batch = (uint32_t)batch;
    p.loader = cfg->loader; p.label = cfg->label; p.n_feat = trsim::loader_features(cfg->loader);
    p.quads = (uint32_t)((size_t)e->H * e->W / 4);                        // W % 4 == 0 -> whole groups of four pixels
    p.frame_dwords = 3 * p.quads;
    const uint32_t units = !plain || cfg->layout == TRS_LAYOUT_NCHW ? p.quads : cfg->dtype == TRS_DTYPE_U8 ? (p.frame_dwords + 3) / 4 : p.frame_dwords;
    if (!trsim::batch_items(p, units)) return trs_internal_fail(TRS_ERR_LIMIT, "batch x frame size beyond 2^31 work items");
    const int grid = (int)std::min<size_t>(p.items, (size_t)e->cu_count * 16);
    if (!plain) trsim::launch_batch_aug(e, p, trsim::AugKey::of(*aug, epoch), (uint32_t)(e->W / 4), cfg->layout, cfg->dtype, grid);
    else if (cfg->layout == TRS_LAYOUT_NHWC) {
        if (cfg->dtype == TRS_DTYPE_F32) launch_batch<TRS_LAYOUT_NHWC, TRS_DTYPE_F32>(e, p, grid);
        else if (cfg->dtype == TRS_DTYPE_F16) launch_batch<TRS_LAYOUT_NHWC, TRS_DTYPE_F16>(e, p, grid);
        else launch_batch<TRS_LAYOUT_NHWC, TRS_DTYPE_U8>(e, p, grid);
    } else {
        if (cfg->dtype == TRS_DTYPE_F32) launch_batch<TRS_LAYOUT_NCHW, TRS_DTYPE_F32>(e, p, grid);
        else launch_batch<TRS_LAYOUT_NCHW, TRS_DTYPE_F16>(e, p, grid);
    }
    HIPCHK(hipGetLastError());
    trsim::resident_note_launch(e);                       // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return TRS_OK;
}

TRS_EXPORT int trs_sample_batch(trs_env* e, const trs_loader_config* cfg, const uint8_t* d_frames, const float* d_rows, int split, int epoch, int first,
                                int batch, void* d_images, float* d_features, float* d_labels, int32_t* d_index)
{
    return trsim::sample_batch(e, cfg, nullptr, d_frames, d_rows, split, epoch, first, batch, d_images, d_features, d_labels, d_index);
}
