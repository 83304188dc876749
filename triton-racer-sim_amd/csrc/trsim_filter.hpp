// trsim_filter.hpp — the static colour filter on the host, as integer and binary32 arithmetic a host compiler builds without HIP: OpenCV's fixed-point
// reciprocal tables (hsv_reciprocals: what the kernels read as `hsv_tab`), ImgPreprocessing.__process of ONE colour (filter_colour: the rasteriser's
// palette is filtered with it) and the argument check of a trs_pre_config (check_pre).  tests/filter_driver.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/trsim.h"

namespace trsim {

// One entry of OpenCV's fixed-point reciprocal tables, hsv_shift = 12: sdiv_table[i] = hsv_reciprocal(255, 1.0, i), hdiv_table180[i] = hsv_reciprocal(180, 6.0, i)
inline int hsv_reciprocal(int range, double sectors, int i) { return i ? (int)std::lrint((range << 12) / (sectors * i)) : 0; }
inline int hsv_sdiv(int v) { return hsv_reciprocal(255, 1.0, v); }
inline int hsv_hdiv(int diff) { return hsv_reciprocal(180, 6.0, diff); }

// sdiv[256] | hdiv[256]: the table the kernels read (PreParams::hsv_tab, FParams::tabs, HillBlock::hsv_tab)
inline void hsv_reciprocals(int tab[512])
{
    for (int i = 0; i < 256; ++i) {
        tab[i] = hsv_sdiv(i);
        tab[256 + i] = hsv_hdiv(i);
    }
}

// what trs_preprocess and trs_set_frame_filter refuse about a trs_pre_config (TRS_ERR_ARG and the text in *why), TRS_OK otherwise
inline int check_pre(const trs_pre_config* c, const char** why)
{
    auto refuse = [&](const char* text) { *why = text; return (int)TRS_ERR_ARG; };
    if (!c || c->struct_size != sizeof(trs_pre_config)) return refuse("trs_pre_config.struct_size mismatch");
    if (c->edge_detection_enabled && (c->edge_dst_channel < 0 || c->edge_dst_channel > 2)) return refuse("edge_dst_channel out of range");
    if (c->n_filters < 0 || c->n_filters > 4) return refuse("n_filters out of range");
    for (int f = 0; f < c->n_filters; ++f)
        if (c->dst_channel[f] < 0 || c->dst_channel[f] > 2) return refuse("dst_channel out of range");
    return TRS_OK;
}

// ImgPreprocessing.__process of ONE colour (img_preprocessing.py:37-74,92-99 without dynamic brightness and Canny):
// the host twin of trs_preprocess_kernel's per-pixel arithmetic, used to filter the rasteriser's palette.
inline uint32_t filter_colour(const trs_pre_config& c, uint32_t bgr)
{
    int t[3];
    for (int ch = 0; ch < 3; ++ch) {
        float x = (float)((bgr >> (8 * ch)) & 255u);
        x = x - c.contrast_offset;
        x = x * c.contrast_ratio;
        x = x + c.contrast_offset;
        x = x < 0.0f ? 0.0f : (x > 255.0f ? 255.0f : x);
        t[ch] = (int)x;
    }
    int o[3] = {t[0], t[1], t[2]};
    if (c.color_filter_enabled) {
        const int r = t[0], g = t[1], b = t[2];
        const int v = std::max(r, std::max(g, b)), vmin = std::min(r, std::min(g, b)), diff = v - vmin;
        const int sdiv = hsv_sdiv(v), hdiv = hsv_hdiv(diff);
        const int sat = (diff * sdiv + (1 << 11)) >> 12;
        int h = (v == r) ? (g - b) : ((v == g) ? (b - r + 2 * diff) : (r - g + 4 * diff));
        h = (h * hdiv + (1 << 11)) >> 12;
        if (h < 0) h += 180;
        const int hh = std::min(h, 255), ss = std::min(sat, 255);
        for (int f = 0; f < c.n_filters; ++f) {
            const bool in = hh >= c.hsv_lo[f][0] && hh <= c.hsv_hi[f][0] && ss >= c.hsv_lo[f][1] && ss <= c.hsv_hi[f][1] &&
                            v >= c.hsv_lo[f][2] && v <= c.hsv_hi[f][2];
            o[c.dst_channel[f]] = in ? 255 : 0;
        }
    }
    return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
}

}  // namespace trsim
