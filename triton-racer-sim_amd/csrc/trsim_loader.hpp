// trsim_loader.hpp — the rules of the training minibatches (include/trsim_spec.h, "training minibatches") in the one place trs_batch_kernel, trs_sample_batch
// and trs_loader_order take them from.  Free of HIP headers, like trsim_expert.hpp: tests/loader_driver.cpp compiles it with a plain host compiler under
// AddressSanitizer + UBSan; under hipcc the arithmetic is __host__ __device__.
//   loader_config_error / loader_range_error / loader_call_error   the refusals of the two calls (nullptr: accepted)
//   mix, perm                                                      the keyed permutation of [0, n)
//   Order                                                          split offsets and keys of one (config, split, epoch): record(p)
//   unit255                                                        a frame byte as float32 / 255
//   loader_features, row_to_sample                                 the row -> features / labels rule
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/trsim.h"
#include "../../include/trsim_spec.h"

#if defined(__HIPCC__)
#define TRS_HD __host__ __device__
#else
#define TRS_HD
#endif

namespace trsim {

constexpr int kLoaderRowFloats = 8;                          // a record row (kExpertRowFloats, trsim_expert.hpp)
enum { kLoaderRowSteer = 0, kLoaderRowThr = 1, kLoaderRowApplied = 3, kLoaderRowSpeed = 4, kLoaderRowSegment = 6 };
constexpr int kLoaderLabels = 2;

inline void loader_defaults(trs_loader_config* c)
{
    c->struct_size = sizeof(trs_loader_config);
    c->loader = TRS_LOADER_SPEED_CTL; c->label = TRS_LABEL_EXPERT; c->layout = TRS_LAYOUT_NCHW; c->dtype = TRS_DTYPE_F32;
    c->n_records = 0; c->n_train = 0;
    c->seed = 0;
}

// F of a loader (-1: no such loader)
TRS_HD inline int loader_features(int loader)
{
    switch (loader) {
    case TRS_LOADER_SPEED_CTL: case TRS_LOADER_DEFAULT: return 0;
    case TRS_LOADER_SPEED_FEATURE: return 1;
    case TRS_LOADER_FULL_HOUSE: return 2;
    }
    return -1;
}

// why this config is refused by either call (nullptr: it is not)
inline const char* loader_config_error(const trs_loader_config* c)
{
    if (!c) return "null trs_loader_config";
    if (c->struct_size != sizeof(trs_loader_config)) return "trs_loader_config.struct_size mismatch";
    if (loader_features(c->loader) < 0) return "trs_loader_config.loader is no TRS_LOADER_* value";
    if (c->label != TRS_LABEL_EXPERT && c->label != TRS_LABEL_APPLIED) return "trs_loader_config.label is no TRS_LABEL_* value";
    if (c->layout != TRS_LAYOUT_NHWC && c->layout != TRS_LAYOUT_NCHW) return "trs_loader_config.layout is no TRS_LAYOUT_* value";
    if (c->dtype != TRS_DTYPE_F32 && c->dtype != TRS_DTYPE_F16 && c->dtype != TRS_DTYPE_U8) return "trs_loader_config.dtype is no TRS_DTYPE_* value";
    if (c->layout == TRS_LAYOUT_NCHW && c->dtype == TRS_DTYPE_U8) return "TRS_LAYOUT_NCHW gives float32 or binary16 only (uint8 frames keep their own order)";
    if (c->n_records < 0) return "trs_loader_config.n_records < 0";
    if (c->n_train < 0 || c->n_train > c->n_records) return "trs_loader_config.n_train must lie in [0, n_records]";
    return nullptr;
}

// the records of a split: split 0 is sigma(0 .. n_train - 1), split 1 is sigma(n_train .. n_records - 1)
TRS_HD inline int split_offset(int n_train, int split) { return split == TRS_SPLIT_TRAIN ? 0 : n_train; }
TRS_HD inline int split_size(int n_records, int n_train, int split) { return split == TRS_SPLIT_TRAIN ? n_train : n_records - n_train; }

// why positions first .. first + count - 1 of (split, epoch) are refused for an accepted config (nullptr: they are not)
inline const char* loader_range_error(const trs_loader_config* c, int split, int epoch, int first, int count)
{
    if (split != TRS_SPLIT_TRAIN && split != TRS_SPLIT_VAL) return "split is no TRS_SPLIT_* value";
    if (epoch < 0) return "epoch < 0";
    if (first < 0 || count < 0) return "first < 0 or a negative number of positions";
    if ((int64_t)first + (int64_t)count > (int64_t)split_size(c->n_records, c->n_train, split)) return "first + batch reaches beyond the split";
    return nullptr;
}

// the pointers of one trs_sample_batch call and whether the handle has a camera
struct LoaderCall {
    const void *frames, *rows, *images, *features, *labels, *index;
    bool render;
};
inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr size_t kImageAlign = 16, kWordAlign = 4;            // the kernel's widest store into d_images; every other array is read or written by dwords

// why trs_sample_batch refuses these pointers for an accepted config (nullptr: it does not)
inline const char* loader_call_error(const trs_loader_config* c, const LoaderCall& k)
{
    if (!k.rows) return "d_rows is NULL";
    if (!k.labels) return "d_labels is NULL";
    if (loader_features(c->loader) > 0 && !k.features) return "d_features is NULL for a loader with features";
    if ((k.frames == nullptr) != (k.images == nullptr)) return "d_frames and d_images go together: both, or neither for a physics-only set";
    if (k.frames && !k.render) return "frames given on a handle without a camera (render == 0)";
    if (k.images && !aligned_to(k.images, kImageAlign)) return "d_images is not 16-byte aligned";
    for (const void* p : {k.frames, k.rows, k.features, k.labels, k.index})
        if (p && !aligned_to(p, kWordAlign)) return "a pointer is not 4-byte aligned";
    return nullptr;
}

// ---- the keyed permutation ----
TRS_HD inline uint64_t mix(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// h = b / 2 of the Feistel network over [0, 2^b) that covers [0, n): b = max(2, bit_length(n - 1)) rounded up to even
TRS_HD inline int perm_half_bits(uint32_t n)
{
    int b = 0;
    for (uint32_t v = n - 1; v; v >>= 1) ++b;                // (n >= 1)
    if (b < 2) b = 2;
    return (b + 1) / 2;
}

TRS_HD inline uint32_t perm(uint64_t key, uint32_t n, uint32_t i, int h)
{
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = i;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (uint64_t r = 0; r < 4; ++r) {
            const uint32_t t = L ^ ((uint32_t)mix(key ^ ((r << 32) | R)) & mask);
            L = R; R = t;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}
TRS_HD inline uint32_t perm(uint64_t key, uint32_t n, uint32_t i) { return perm(key, n, i, perm_half_bits(n)); }

// one (config, split, epoch): record(p) = sigma(off_s + perm(K_e,s, n_s, p)) for p in [0, n_s)
struct Order {
    uint64_t key_split, key_epoch;
    uint32_t n, n_s, off;
    int h, h_s;
    TRS_HD static Order of(uint64_t seed, int n_records, int n_train, int split, int epoch)
    {
        Order o;
        o.key_split = mix(seed);
        o.key_epoch = mix(o.key_split ^ (((uint64_t)(uint32_t)(split + 1) << 32) | (uint64_t)(uint32_t)epoch));
        o.n = (uint32_t)n_records; o.n_s = (uint32_t)split_size(n_records, n_train, split); o.off = (uint32_t)split_offset(n_train, split);
        o.h = perm_half_bits(o.n ? o.n : 1u); o.h_s = perm_half_bits(o.n_s ? o.n_s : 1u);
        return o;
    }
    TRS_HD uint32_t record(uint32_t p) const { return perm(key_split, n, off + perm(key_epoch, n_s, p, h_s), h); }
};

// ---- a frame byte -> [0, 1] ----
// (float)v / 255.0f for v in 0 .. 255 without the division's instruction sequence: the quotient by the reciprocal, then one Newton step on the exact
// remainder (two fused multiply-adds, written out: they are the algorithm, not a contraction).  tests/test_loader_cpu.py compares all 256 values with the
// IEEE division bit for bit.
TRS_HD inline float unit255(uint32_t v)
{
    const float x = (float)v, r = 1.0f / 255.0f;
    const float q = x * r;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), r, q);
}

// ---- row -> features, labels ----
struct Sample { float feat[2], label[kLoaderLabels]; };
TRS_HD inline Sample row_to_sample(const float* row, int loader, int label)
{
    Sample s;
    const float steer = row[label == TRS_LABEL_APPLIED ? kLoaderRowApplied : kLoaderRowSteer];
    const float s20 = (float)((double)row[kLoaderRowSpeed] / 20.0);
    s.feat[0] = s20; s.feat[1] = row[kLoaderRowSegment];
    s.label[0] = steer;
    s.label[1] = (loader == TRS_LOADER_SPEED_CTL || loader == TRS_LOADER_FULL_HOUSE) ? s20 : row[kLoaderRowThr];
    return s;
}

}  // namespace trsim
