// trsim_jpeg_host.hpp — what the entry points of trsim_jpeg.hip, trsim_jpeg_decode.hip and trsim_jpeg_codec.hip check and report alike (host only).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "trsim_env.hpp"
#include "trsim_internal.hpp"

namespace trsim {
namespace jpeg {

// what a call that takes a quality and a number of images refuses first, in this order
inline int check_call(const trs_env* e, int n_images, int quality)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (quality < 1 || quality > 100) return trs_internal_fail(TRS_ERR_ARG, "quality must be in [1, 100]");
    if (n_images < 1) return trs_internal_fail(TRS_ERR_ARG, "n_images < 1");
    return TRS_OK;
}

// a NULL *d_src stands for the handle's latest frames, n_envs of them; what: the call's use of them, as the refusal of a handle without a camera ends
inline int latest_frame_source(const trs_env* e, int n_images, const char* what, const uint8_t** d_src)
{
    if (*d_src) return TRS_OK;
    *d_src = trs_internal_latest_frame(e);
    if (!*d_src) return trs_internal_fail(TRS_ERR_STATE, std::string("the env has no camera (cfg.render == 0): there is no latest frame ") + what);
    if (n_images != e->n) return trs_internal_fail(TRS_ERR_ARG, "latest-frame source needs n_images == n_envs");
    return TRS_OK;
}

// the handle's buffers for `bytes` of `what` could not be reserved
inline int no_memory(hipError_t rh, size_t bytes, const char* what)
{
    return trs_internal_fail(rh == hipErrorOutOfMemory ? TRS_ERR_NOMEM : TRS_ERR_DEVICE, "no memory for " + std::to_string(bytes) + " bytes of " + what);
}

}  // namespace jpeg
}  // namespace trsim
