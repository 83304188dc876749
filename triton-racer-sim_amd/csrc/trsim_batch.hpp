// trsim_batch.hpp — what the two minibatch kernels share (trs_batch_kernel, trsim_loader.hip; trs_batch_aug_kernel, trsim_augment.hip): the work
// decomposition's constants, the parameters of one launch, the 4-byte-aligned wide access types and the 4-value store of one unit.  Device code: HIP only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/trsim.h"
#include "trsim_augment.hpp"
#include "trsim_loader.hpp"

struct trs_env;

namespace trsim {

constexpr int kBatchBlock = 256, kBatchUnroll = 4, kUnitsPerItem = kBatchBlock * kBatchUnroll;

struct BatchParams {
    const uint32_t* frames;             // the set's frames as dwords, or nullptr (physics-only set)
    const float* rows;
    void* images; float* features; float* labels; int32_t* index;
    trsim::Order order;
    uint32_t first, batch;
    int loader, label, n_feat;
    uint32_t frame_dwords, quads;       // H * W * 3 / 4 and H * W / 4
    uint32_t units, chunks;             // units of a frame in this layout, and items per slot
    uint32_t items;                     // batch * chunks
};

__device__ __forceinline__ float unit8(uint32_t v) { return trsim::unit255(v); }

// three and four dwords of a frame in one load (and, for uint8 output, one store): the address is a multiple of 4 and no more
typedef uint32_t dwords3_t __attribute__((ext_vector_type(3)));
typedef uint32_t dwords4_t __attribute__((ext_vector_type(4)));
typedef dwords3_t __attribute__((aligned(4))) dwords3_a4;
typedef dwords4_t __attribute__((aligned(4))) dwords4_a4;
__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }
__device__ __forceinline__ uint32_t half_bits(float f) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)f); }   // round to nearest even
__device__ __forceinline__ uint2 halves4(float a, float b, float c, float d)
{
    return make_uint2(half_bits(a) | (half_bits(b) << 16), half_bits(c) | (half_bits(d) << 16));
}

// four values of one unit, in output order, to element e of an array of 4-element groups
template <int DTYPE>
__device__ __forceinline__ void store4(void* base, size_t e, uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    if (DTYPE == TRS_DTYPE_F32) static_cast<float4*>(base)[e] = make_float4(unit8(b0), unit8(b1), unit8(b2), unit8(b3));
    else if (DTYPE == TRS_DTYPE_F16) static_cast<uint2*>(base)[e] = halves4(unit8(b0), unit8(b1), unit8(b2), unit8(b3));
    else static_cast<uint32_t*>(base)[e] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// the items of one launch over `units` units per frame (one item per slot for a physics-only set); false: beyond 2^31 work items
inline bool batch_items(BatchParams& p, uint32_t units)
{
    p.units = units;
    p.chunks = p.frames ? (p.units + kUnitsPerItem - 1) / kUnitsPerItem : 1;
    const size_t items = (size_t)p.batch * p.chunks;
    if (items > 0x7FFFFFFFu) return false;
    p.items = (uint32_t)items;
    return true;
}

// trsim_loader.hip: the one path of trs_sample_batch (aug == nullptr) and trs_sample_batch_aug
int sample_batch(trs_env* e, const trs_loader_config* cfg, const trs_augment_config* aug, const uint8_t* d_frames, const float* d_rows, int split, int epoch,
                 int first, int batch, void* d_images, float* d_features, float* d_labels, int32_t* d_index);

// trsim_augment.hip: one launch of trs_batch_aug_kernel<layout, dtype> on the handle's stream; p.units == p.quads, `row_quads` = W / 4
void launch_batch_aug(const trs_env* e, const BatchParams& p, const AugKey& key, uint32_t row_quads, int layout, int dtype, int grid);

}  // namespace trsim
