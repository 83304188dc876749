// trsim_augment.hip — the augmented training minibatches of libtrsim.so (include/trsim_spec.h, "training minibatches, augmentation"): trs_sample_batch's
// gather with a mirror and a colour jitter per record applied on the way through, so that a training loop varies a record between epochs without another
// pass over the float batch.  One kernel, trs_batch_aug_kernel; the rules (refusals, the keyed draw) are trsim_augment.hpp, shared with
// trs_loader_augment, which gives the same draws on the host without a GPU; the pixel rule is light_channel (trsim_tables.hpp), the one the rasteriser
// lights palette entries with.
//
// Work items as in trs_batch_kernel (trsim_loader.hip): (batch slot, chunk of kUnitsPerItem units), the grid sized from the CU count and striding over
// the items, the record number a function of the workgroup's index alone.  The draw is keyed by the record, so it is wave-uniform too: the eight mix
// calls run once per item, and the mirror branch is taken by whole waves.
// The unit is FOUR PIXELS (12 bytes, one load at a 4-byte aligned address) in every layout: W % 4 == 0, so a row is whole units, and output unit c of a
// mirrored row is input unit W/4 - 1 - c with its four pixels in reverse order — byte picks in registers, no LDS.  Lanes take consecutive output units,
// so a wave's loads cover one contiguous run (walking downwards within a mirrored row; a wave that spans rows has one run per row), and so do
//   NCHW        one 16-B (float32) or 8-B (binary16) store into each of the three planes
//   NHWC uint8  one 12-B store, typed 4-byte aligned like the load
// NHWC float32 / binary16 is where an instruction does NOT cover a contiguous run: a lane owns 12 consecutive values and writes them with three 16-B
// (8-B) stores, so each store instruction of a wave touches 16 of every 48 bytes (8 of 24) and the three together fill the run.  Measured at 1024
// slots of 120 x 160 against trs_batch_kernel of the same layout and type (profiles/r29_augment.txt): float32 NHWC 1.34 x (the 1.25 x line MISSED;
// binary16 NHWC 0.96 x), where float32 NCHW is 1.03 x, binary16 NCHW 1.19 x and uint8 NHWC 1.24 x.
// The row of a unit is needed on mirrored records only, and is found without a division: y = mulhi(u, floor(2^32 / (W/4))) is the row or one less (the
// product falls short of u / (W/4) by less than u / 2^32 < 1), one conditional subtraction corrects it.
// Frame starts are multiples of 4 bytes and no more (trsim_loader.hip): the wide accesses are typed 4-byte aligned.  No LDS, no atomics, no per-handle
// state.  The features, labels (label[0] with its sign bit flipped on a mirrored record) and record number of a slot are written by lane 0 of the slot's
// first item.  Bound: HBM, the bytes of trs_batch_kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/trsim.h"
#include "trsim_augment.hpp"
#include "trsim_batch.hpp"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"

namespace {

using namespace trsim;

struct AugParams {
    AugKey key;
    uint32_t row_quads, row_magic;      // W / 4 and floor(2^32 / row_quads) (2^32 - 1 for row_quads == 1)
};

// kBatchUnroll units of one item: unit u of the output is unit `su` of the record's frame, lit, with its pixels reversed on a mirrored record
template <int LAYOUT, int DTYPE, bool MIRROR>
__device__ __forceinline__ void aug_units(const BatchParams& p, const AugParams& a, const float* gb, const uint32_t* src, uint32_t slot, uint32_t chunk)
{
#pragma unroll
    for (int k = 0; k < kBatchUnroll; ++k) {
        const uint32_t u = chunk * kUnitsPerItem + k * kBatchBlock + threadIdx.x;
        if (u >= p.units) continue;
        uint32_t su = u;
        if (MIRROR) {
            uint32_t c = u - __umulhi(u, a.row_magic) * a.row_quads;         // the column, or the column + row_quads
            if (c >= a.row_quads) c -= a.row_quads;
            su = u + a.row_quads - 1 - 2 * c;                                // the same row, column row_quads - 1 - c
        }
        const dwords3_a4 w = *reinterpret_cast<const dwords3_a4*>(src + 3 * (size_t)su);
        const uint32_t in[3] = {w.x, w.y, w.z};                              // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        uint32_t o[12];                                                      // the output unit's bytes, in the frame's own order
#pragma unroll
        for (int px = 0; px < 4; ++px)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int j = 3 * (MIRROR ? 3 - px : px) + c;
                o[3 * px + c] = light_channel(byte_of(in[j / 4], j % 4), gb[c], gb[4 + c]);
            }
        if (LAYOUT == TRS_LAYOUT_NCHW) {
            const size_t e = (size_t)slot * 3 * p.quads + u;
            store4<DTYPE>(p.images, e, o[0], o[3], o[6], o[9]);
            store4<DTYPE>(p.images, e + p.quads, o[1], o[4], o[7], o[10]);
            store4<DTYPE>(p.images, e + 2 * (size_t)p.quads, o[2], o[5], o[8], o[11]);
        } else if (DTYPE == TRS_DTYPE_U8) {
            dwords3_t v;
            v.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            v.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
            v.z = o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24);
            *reinterpret_cast<dwords3_a4*>(static_cast<uint32_t*>(p.images) + (size_t)slot * p.frame_dwords + 3 * (size_t)u) = v;
        } else {
            const size_t e = (size_t)slot * p.frame_dwords + 3 * (size_t)u;
            store4<DTYPE>(p.images, e, o[0], o[1], o[2], o[3]);
            store4<DTYPE>(p.images, e + 1, o[4], o[5], o[6], o[7]);
            store4<DTYPE>(p.images, e + 2, o[8], o[9], o[10], o[11]);
        }
    }
}

template <int LAYOUT, int DTYPE>
__global__ __launch_bounds__(kBatchBlock) void trs_batch_aug_kernel(const BatchParams p, const AugParams a)
{
    for (uint32_t item = blockIdx.x; item < p.items; item += gridDim.x) {
        const uint32_t slot = item / p.chunks, chunk = item - slot * p.chunks;
        const uint32_t rec = p.order.record(p.first + slot);                 // wave-uniform, and so is the draw
        const AugDraw d = a.key.draw(rec);
        if (chunk == 0 && threadIdx.x == 0) {
            const Sample s = row_to_sample(p.rows + (size_t)rec * kLoaderRowFloats, p.loader, p.label);
            for (int f = 0; f < p.n_feat; ++f) p.features[(size_t)slot * p.n_feat + f] = s.feat[f];
            const uint32_t steer = __builtin_bit_cast(uint32_t, s.label[0]) ^ (d.mirror << 31);
            p.labels[(size_t)slot * 2] = __builtin_bit_cast(float, steer); p.labels[(size_t)slot * 2 + 1] = s.label[1];
            if (p.index) p.index[slot] = (int32_t)rec;
        }
        if (!p.frames) continue;
        const uint32_t* src = p.frames + (size_t)rec * p.frame_dwords;
        if (d.mirror) aug_units<LAYOUT, DTYPE, true>(p, a, d.gb, src, slot, chunk);
        else aug_units<LAYOUT, DTYPE, false>(p, a, d.gb, src, slot, chunk);
    }
}

template <int LAYOUT, int DTYPE>
void launch_aug(const trs_env* e, const BatchParams& p, const AugParams& a, int grid)
{
    hipLaunchKernelGGL((trs_batch_aug_kernel<LAYOUT, DTYPE>), dim3(grid), dim3(kBatchBlock), 0, e->sP, p, a);
}

}  // namespace

void trsim::launch_batch_aug(const trs_env* e, const BatchParams& p, const AugKey& key, uint32_t row_quads, int layout, int dtype, int grid)
{
    AugParams a;
    a.key = key;
    a.row_quads = row_quads;
    a.row_magic = row_quads == 1 ? 0xFFFFFFFFu : (uint32_t)(0x100000000ull / row_quads);
    if (layout == TRS_LAYOUT_NHWC) {
        if (dtype == TRS_DTYPE_F32) launch_aug<TRS_LAYOUT_NHWC, TRS_DTYPE_F32>(e, p, a, grid);
        else if (dtype == TRS_DTYPE_F16) launch_aug<TRS_LAYOUT_NHWC, TRS_DTYPE_F16>(e, p, a, grid);
        else launch_aug<TRS_LAYOUT_NHWC, TRS_DTYPE_U8>(e, p, a, grid);
    } else {
        if (dtype == TRS_DTYPE_F32) launch_aug<TRS_LAYOUT_NCHW, TRS_DTYPE_F32>(e, p, a, grid);
        else launch_aug<TRS_LAYOUT_NCHW, TRS_DTYPE_F16>(e, p, a, grid);
    }
}

TRS_EXPORT void trs_default_augment_config(trs_augment_config* aug)
{
    if (aug) trsim::augment_defaults(aug);
}

TRS_EXPORT int trs_sample_batch_aug(trs_env* e, const trs_loader_config* cfg, const trs_augment_config* aug, const uint8_t* d_frames, const float* d_rows,
                                    int split, int epoch, int first, int batch, void* d_images, float* d_features, float* d_labels, int32_t* d_index)
{
    return trsim::sample_batch(e, cfg, aug, d_frames, d_rows, split, epoch, first, batch, d_images, d_features, d_labels, d_index);
}

TRS_EXPORT int trs_loader_augment(const trs_loader_config* cfg, const trs_augment_config* aug, int split, int epoch, int first, int count, int32_t* h_index,
                                  uint8_t* h_mirror, float* h_params)
{
    if (const char* why = trsim::loader_config_error(cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (const char* why = trsim::loader_range_error(cfg, split, epoch, first, count)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (const char* why = trsim::augment_config_error(aug, cfg)) return trs_internal_fail(TRS_ERR_ARG, why);
    if (count > 0 && (!h_mirror || !h_params)) return trs_internal_fail(TRS_ERR_ARG, "h_mirror or h_params is NULL");
    const trsim::Order o = trsim::Order::of(cfg->seed, cfg->n_records, cfg->n_train, split, epoch);
    const trsim::AugKey key = trsim::AugKey::of(*aug, epoch);
    for (int k = 0; k < count; ++k) {
        const uint32_t rec = o.record((uint32_t)(first + k));
        const trsim::AugDraw d = key.draw(rec);
        if (h_index) h_index[k] = (int32_t)rec;
        h_mirror[k] = (uint8_t)d.mirror;
        for (int j = 0; j < trsim::kAugmentParams; ++j) h_params[(size_t)k * trsim::kAugmentParams + j] = d.gb[j];
    }
    return TRS_OK;
}
