// trsim_pilot_plan.hpp — which kernel serves which layer of the pilot, and how its weights are packed, as arithmetic a host compiler builds without HIP:
// the layer geometry of Keras_2D_CNN for a frame size, the kernel of every layer with its LDS layout (pilot_plan), what a call of n frames adds to it
// (dense_call, head_call, the grids), the constants the plan shares with the kernels, the packing of the Keras arrays into fp16 granules, and the
// blob of small fp32 weights the tail kernels read (its slots XO_*, the branch widths, pack_tail_blob).
// No device pointer lives here: trsim_pilot_pass.hpp fills the kernels' parameter blocks and schedules a pass from a PilotPlan.  tests/pilot_plan_driver.cpp runs both on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/trsim.h"

#ifndef TRS_FRAME_LOADERS
#define TRS_FRAME_LOADERS 4   /* loader waves of trs_conv_frame_kernel beside its 8 compute waves */
#endif
#ifndef TRS_F5_COMPUTE
#define TRS_F5_COMPUTE 4   /* compute waves of trs_conv_frame5_kernel (+ 4 loader waves); 1 x 8 and 2 x 8 measured: see the kernel */
#endif

namespace trsim {

constexpr int kPilotLds = 160 * 1024, kPilotLdsDb = 158 * 1024;   // LDS of a CU: no launch asks for more; what the double-buffered kernels (frame, frame5, chain) may plan with
constexpr int kBandPf = 2;                 // 16-byte chunks of the band per loader thread of trs_conv12_band_kernel (waves 8..15: 512 threads; 4 until round 2:
                                           // the 8 registers now hold conv1's bias)
constexpr int kDenseChunk = 72;            // granules per LDS chunk of trs_pilot_dense_kernel = 36 k-steps
constexpr int kDensePitch = 73;            // LDS row pitch in granules (odd: 16 lanes cover all 64 banks)
constexpr int kDenseLds = 2 * 32 * kDensePitch * 16;   // per 32 frames (NF = 2: twice that)
constexpr int kFrameBlock = 64 * (8 + TRS_FRAME_LOADERS), kFrame5Block = 64 * (TRS_F5_COMPUTE + 4), kChainBlock = 512;
// floor(p / d) = umulhi(p, pilot_magic(d)), exact for p < 2^32 / d: the kernels' item set-up without divisions.  d >= 2: for d = 1 the factor would be 2^32,
// which comes back as 0 (every quotient 0) — the plan keeps a layer whose divisor would be 1 off the kernels that divide this way (plan_frame)
inline unsigned pilot_magic(int d) { return (unsigned)((0x100000000ull + (unsigned)d - 1u) / (unsigned)d); }

inline trs_pilot_tuning pilot_default_tuning()
{
    trs_pilot_tuning t{};
    t.struct_size = (uint32_t)sizeof t; t.fuse_band_r2 = 6; t.fuse_wsplit_max = 4; t.span_layers_mask = 0x6;
    t.fuse_roll = 1; t.frame5 = 1; t.frame_layers_mask = 0x78; t.chain_layers = 4; t.dense = 1;
    return t;
}

// ---- the plan of a loaded model ---------------------------------------------------------------------------------------------------
struct PilotLayer {
    int KH = 0, KW = 0, S = 0, CIN = 0, COUT = 0, COUT_PAD = 0, IH = 0, IW = 0, OH = 0, OW = 0, G = 0, G_pad = 0, run = 0, run_pad = 0;   // run: granules of a kernel row, run_pad: padded to whole trips of 4
    bool u8in = false, out_f32 = false, relu = true;
    // conv1..7 on the single-layer kernels (trs_conv_u8_kernel, trs_conv_lt_kernel, trs_conv_span_kernel): the weights (or a 64-channel
    // slice) live in LDS, persistent workgroups
    int res_nb = 1, res_ysplit = 1, res_lds = 0, res_block = 512, res_wg_per_cu = 1;
    bool res_span = false; int span_nl = 0;                                               // trs_conv_span_kernel (stride-2 5x5 layers: per-row input spans staged in LDS)
    bool frame = false; int frame_f = 1, frame_lds = 0, frame_bands = 1, frame_ohb = 0;   // trs_conv_frame_kernel (3x3 stride-1 layers: F frames' input activations in LDS)
    bool frame5 = false; int frame5_lds = 0, frame5_bands = 1, frame5_ohb = 0;            // trs_conv_frame5_kernel (conv3: one input frame / band per workgroup in LDS)
    size_t act_elems() const { return (size_t)OH * OW * COUT; }                          // per frame
};
struct PilotHead {                         // conv1 -> conv2 in one kernel, band form (trs_conv12_band_kernel): conv1's activation stays in LDS
    bool on = false;
    int R2 = 0, bands = 0, wsplit = 0, w2p = 0, cpr = 0;   // conv2 rows per band, bands per frame; parts in width (1: whole), conv2 columns per part, 16-byte chunks per staged row
    int off_w2 = 0, off_b = 0, off_tile = 0, off_band = 0, tile_bytes = 0, band_bytes = 0, lds = 0;
    unsigned magic_full = 0, magic_cpr = 0;
};
struct PilotChain {                        // conv(first + 1) .. conv7 in one launch (trs_conv_chain_kernel); first = -1: layer by layer
    int first = -1, nl = 0, F = 0, split_first = 0, offA = 0, offB = 0, off_bias = 0, lds = 0;
    int nt[4] = {}, nb[4] = {};
    unsigned magic_uout[4] = {}, magic_ow[4] = {};
};
struct PilotPlan {
    int err = TRS_OK; const char* err_text = nullptr;     // a refusal: nothing else of the plan is valid
    int H = 0, W = 0, n_cap = 0, cu_count = 256, arch = TRS_PILOT_SPD_CTL, n_layers = 8;
    trs_pilot_tuning tun{};
    PilotLayer L[9];                       // conv1..7 + dense1 (1x1 "conv" over frames) [+ dense4: the second head of cnn_2d_full_house]
    PilotHead head;
    PilotChain chain;
};
// layer i of Keras_2D_CNN over an ih x iw input (i >= 7: dense1 / dense4 over the NHWC flatten of conv7's ih x iw output)
inline PilotLayer pilot_layer_geometry(int i, int ih, int iw)
{
    static const int spec[7][4] = {{5, 2, 3, 24}, {5, 2, 24, 32}, {5, 2, 32, 64}, {3, 1, 64, 64}, {3, 1, 64, 64}, {3, 1, 64, 128}, {3, 1, 128, 128}};
    PilotLayer l;
    if (i < 7) { l.KH = l.KW = spec[i][0]; l.S = spec[i][1]; l.CIN = spec[i][2]; l.COUT = spec[i][3]; l.IH = ih; l.IW = iw; }
    else { l.KH = l.KW = 1; l.S = 1; l.CIN = ih * iw * 128; l.COUT = 100; l.IH = 1; l.IW = 1; }       // the kernel's first CIN rows; the rows of the small branches go to the tail
    l.OH = (l.IH - l.KH) / l.S + 1; l.OW = (l.IW - l.KW) / l.S + 1;
    l.COUT_PAD = (l.COUT + 31) / 32 * 32;
    l.u8in = (i == 0); l.relu = true; l.out_f32 = (i >= 7);
    // granules: a kernel row is one contiguous run of KW * CIN / 8 granules in NHWC; runs are padded to whole trips of 4
    // (zero weights) so that a trip is always 64 contiguous bytes (trs_conv_lt_kernel); dense1 is one long run
    l.run = l.u8in ? 2 : l.KW * l.CIN / 8; l.run_pad = l.u8in ? 2 : (l.run + 3) & ~3;
    l.G = l.KH * l.run_pad;
    l.G_pad = (l.G + 3) & ~3;
    return l;
}
// conv layers on their single-layer kernels: resident weights, at most 64 output channels per slice (NB <= 2 keeps 16 waves per CU in registers)
inline bool plan_single(PilotLayer& l, int i, const trs_pilot_tuning& T)
{
    l.res_nb = std::min(2, l.COUT_PAD / 32);
    l.res_ysplit = l.COUT_PAD / (32 * l.res_nb);
    // stride-2 layers with wide kernels re-fetch every byte ~2.5x through overlapping windows: span staging instead
    const int cgr = l.CIN / 8, pix_gran = l.S * cgr;
    const int nseg_max = 30 / l.OW + 2;
    // (span_layers_mask: bit i = conv(i+1) uses the span kernel: conv2 and conv3, 0x6; whole 32-channel blocks: its epilogue stores 16 channels per lane)
    l.res_span = !l.u8in && l.S == 2 && l.KW >= 5 && nseg_max <= 4 && ((T.span_layers_mask >> i) & 1) && l.COUT % 32 == 0;
    if (l.res_span) {
        l.span_nl = ((32 - nseg_max) * pix_gran + nseg_max * l.run_pad + 63) / 64;
        if (l.span_nl > 5) l.res_span = false;
    }
    const int stage_per_wave = l.res_span ? l.span_nl * 1024 : 2048;  // input transpose / span stage; output transpose (all kernels)
    auto lds_for = [&](int nb, int waves) { return l.G_pad * nb * 32 * 16 + ((l.G_pad * 4 + 15) & ~15) + nb * 32 * 4 + waves * stage_per_wave; };
    // conv7's 64-channel slices at 7 waves beat 32-channel slices at 16 (240x320: 199 -> 143 us; the pixels are read twice instead of four times)
    if (lds_for(l.res_nb, 7) > kPilotLds) { l.res_nb = 1; l.res_ysplit = l.COUT_PAD / 32; }    // 32-channel slices
    if (lds_for(l.res_nb, 4) > kPilotLds) return false;
    // workgroups per CU and waves per workgroup: about 16 waves per CU when LDS allows
    l.res_wg_per_cu = 1;
    for (int wg = 4; wg >= 1; --wg) {
        const int waves = std::max(4, 16 / wg);
        if (wg * (lds_for(l.res_nb, waves) + 512) <= kPilotLds) { l.res_wg_per_cu = wg; break; }
    }
    int waves = std::max(4, 16 / l.res_wg_per_cu);
    if (l.res_span) waves = std::min(waves, 12);                      // trs_conv_span_kernel is built for <= 768 threads
    while (waves > 4 && l.res_wg_per_cu * (lds_for(l.res_nb, waves) + 512) > kPilotLds) --waves;
    l.res_block = 64 * waves;
    l.res_lds = lds_for(l.res_nb, waves);
    return true;
}
// conv4..7: frames in LDS when they fit (240x320: conv7's 167 KB frame does not: the quad-load kernel stays)
inline void plan_frame(PilotLayer& l, int n_cap, int cu_count)
{
    const int cg = l.CIN / 8;
    // OW >= 2: the frame kernel and the chain divide a pixel index by OW (and by the unit's pixels, a multiple of it) through pilot_magic, which has no
    // 32-bit value for a divisor of 1.  conv7 is one pixel wide for frames 96 and 100 wide: the quad-load kernel takes it, and no chain is built
    const bool shape_ok = l.S == 1 && l.KH == 3 && l.KW == 3 && (cg == 8 || cg == 16) && l.COUT_PAD % 64 == 0 && l.COUT == l.COUT_PAD && l.run_pad == l.KW * cg && l.OW >= 2;
    if (!shape_ok) return;
    // Two LDS buffers (the group being computed and the next one), F units each, a unit = a frame or one of `bands` row bands of it (240x320:
    // conv4 128 KB, conv6 97 KB, conv7 167 KB per frame).  Among the (bands, F) that fit, take the one with the fewest MFMA rounds: a group is
    // ceil(tiles / 2) x (COUT / 64) wave items for 8 compute waves; bands re-stage KH - 1 rows each (a small penalty), every CU should get
    // at least two groups (one to compute, one on its way).
    int bands = 1, f = 1; double best = 1e30;
    for (int bnd = 1; bnd <= l.OH && bnd <= 8; ++bnd) {
        const int ohb_ = (l.OH + bnd - 1) / bnd;
        const size_t unit_ = (size_t)(ohb_ + l.KH - 1) * l.IW * l.CIN * 2;
        for (int f_ = 1; f_ <= 8; ++f_) {
            if (2 * unit_ * f_ + l.COUT_PAD * 4 > (size_t)kPilotLdsDb) break;
            const long groups = ((long)n_cap * bnd + f_ - 1) / f_;
            if (f_ > 1 && groups < 2 * cu_count) break;
            const int tiles = (f_ * ohb_ * l.OW + 31) / 32, items = ((tiles + 1) / 2) * (l.COUT_PAD / 64);
            const double rounds = (double)((items + 7) / 8), per_cu = std::ceil((double)groups / cu_count);
            const double cost = per_cu * (rounds + 0.15) * (1.0 + 0.1 * (double)(bnd - 1) * (l.KH - 1) / l.OH);   // + a barrier and a hand-over per group
            if (cost < best - 1e-9) { best = cost; bands = bnd; f = f_; }
        }
    }
    const int ohb = (l.OH + bands - 1) / bands;
    const size_t unit_bytes = (size_t)(ohb + l.KH - 1) * l.IW * l.CIN * 2;
    l.frame = best < 1e29;
    l.frame_f = f; l.frame_bands = bands; l.frame_ohb = ohb; l.frame_lds = (int)(2 * f * unit_bytes) + l.COUT_PAD * 4;
}
// conv3: frames in LDS when two fit (120x160: 2 x 64 KB); trs_pilot_tuning.frame5 = 0: the span kernel
inline void plan_frame5(PilotLayer& l)
{
    const bool shape_ok = l.KH == 5 && l.KW == 5 && l.S == 2 && l.CIN == 32 && l.COUT == 64 && l.COUT_PAD == 64 && l.run_pad == 20 && l.G_pad == 100;
    // a frame larger than ~78 KB is cut into row bands (240x320: 57 x 77 x 32 = 281 KB -> 5 bands of 6 output rows = 15 input rows, 74 KB)
    int bands = 1;
    while (bands < l.OH && (size_t)(bands == 1 ? l.IH : 2 * ((l.OH + bands - 1) / bands) + 3) * l.IW * 64 > 78 * 1024) ++bands;
    const int ohb = (l.OH + bands - 1) / bands, ihb = bands == 1 ? l.IH : 2 * ohb + 3;
    const size_t unit = (size_t)ihb * l.IW * 64;
    // (row bands at 240x320: 89 us against the span kernel's 86 in round 3, one unit per workgroup; 72.0 against 83.1 on the persistent double-buffered
    // workgroup of round 4: bands by default where a frame does not fit)
    if (shape_ok && 2 * unit + 256 <= (size_t)kPilotLdsDb) {          // two buffers: the unit being computed and the next one
        l.frame5 = true; l.frame5_lds = (int)(2 * unit) + 64 * 4; l.frame5_bands = bands; l.frame5_ohb = ohb;
    }
}
// conv1 -> conv2 fusion: needs the 5x5/2 + 5x5/2 head of Keras_2D_CNN and an LDS tile of 2 R2 + 3 conv1 rows
inline PilotHead plan_head(const PilotLayer& l0, const PilotLayer& l1, const trs_pilot_tuning& T)
{
    PilotHead q;
    const bool shape_ok = l0.G_pad == 12 && l0.COUT_PAD == 32 && l1.G_pad == 80 && l1.COUT_PAD == 32 && l1.COUT == 32 && l1.CIN == 24 && l1.S == 2 && l1.KH == 5;
    const bool band_ok = l0.OW >= 32 && (2 * 8 + 3) * l0.OW < 65536;   // the band kernels split a tile's first pixel on the scalar unit and let a lane wrap once
    // the LDS of a band of r2 conv2 rows: both layers' weights, conv1's bias, the conv1 tile (two column-parity planes per row) and the staged frame rows
    auto layout = [&](int r2, int tile_cols, int band_bytes) {
        PilotHead h;
        int off = 12 * 32 * 16;
        h.off_w2 = off; off += 80 * 32 * 16;
        h.off_b = off; off += 16 * 16;
        h.off_tile = off; h.tile_bytes = (((2 * r2 + 3) * 2 * tile_cols * 48 + 128) + 15) & ~15; off += h.tile_bytes;
        h.off_band = off; h.band_bytes = band_bytes; off += h.band_bytes;
        h.lds = off; h.R2 = r2; h.bands = (l1.OH + r2 - 1) / r2;
        h.on = off <= kPilotLds;
        return h;
    };
    // band form (conv1's input staged once per band as a fp16 image): tile + band image
    // (measured, 1024 frames of 120x160: R2 = 7 / 6 / 5 -> 129 / 114 / 125 us against 131 for the direct form; 512 frames of
    // 240x320, where only R2 = 2 fits: 290 against 272 - bands thinner than 4 rows recompute too much of conv1)
    const int band_r2 = T.fuse_band_r2;                               // 6; 0 = never fuse
    for (int r2 = std::min(band_r2, l1.OH); shape_ok && band_ok && r2 >= std::min(4, l1.OH); --r2) {
        const int rows_in = 2 * (2 * r2 + 3) + 3, row_in = l0.IW * 3;
        if (row_in % 16 != 0 || rows_in * row_in > kBandPf * 512 * 16) continue;
        q = layout(r2, (l0.OW + 1) / 2, rows_in * row_in * 2 + 64);
        if (q.on) { q.wsplit = 1; return q; }
    }
    // the band cut in width (240x320: a whole-width band does not fit): parts of w2p conv2 columns, each with its own conv1 tile and
    // staged frame-row segments (a part re-stages 2 x 3 + 3 input columns and recomputes 3 conv1 columns of its neighbour)
    const int max_split = T.fuse_wsplit_max;                          // 4; 1 = never cut in width
    for (int ws = 2; shape_ok && band_r2 > 0 && ws <= max_split; ++ws) {
        const int w2p = (l1.OW + ws - 1) / ws, w1m = 2 * w2p + 3;          // every part w2p conv2 columns wide (the last one overlaps its neighbour)
        if (w2p < 15 || w2p > l1.OW || w1m * 19 >= 65536) continue;
        const int cpr = ((2 * w1m + 3) * 3 + 15) / 16;
        for (int r2 = std::min(band_r2, l1.OH); r2 >= std::min(4, l1.OH); --r2) {
            const int rows_in = 2 * (2 * r2 + 3) + 3;
            if (rows_in * cpr > kBandPf * 512) continue;
            q = layout(r2, w2p + 2, rows_in * cpr * 32 + 64);
            if (!q.on) continue;
            q.wsplit = ws; q.w2p = w2p; q.cpr = cpr; q.magic_full = pilot_magic(w1m); q.magic_cpr = pilot_magic(cpr);
            return q;
        }
    }
    return PilotHead{};
}
// conv4..conv7 (or conv5..conv7) as one launch when F frames of all their activations fit LDS; trs_pilot_tuning.chain_layers = 0: off, 3 / 4: layers
inline PilotChain plan_chain(const PilotLayer* L, int n_cap, int cu_count, const trs_pilot_tuning& T)
{
    for (int nl = std::min(T.chain_layers, 4); nl >= 3; --nl) {
        const int first = 7 - nl;
        bool ok = true;
        for (int i = first; i < 7; ++i) {
            const PilotLayer& l = L[i];
            ok = ok && l.frame && l.COUT == l.COUT_PAD && l.CIN == (i == 6 ? 128 : 64) && (l.COUT == 64 || l.COUT == 128);
        }
        if (!ok) continue;
        auto out_bytes = [&](int i) { return (size_t)L[i].OH * L[i].OW * L[i].COUT * 2; };
        auto in_bytes_of = [&](int i) { return (size_t)L[i].IH * L[i].IW * L[i].CIN * 2; };
        for (int f = 4; f >= 2; f -= 2) {
            if (f > 2 && (n_cap + f - 1) / f < cu_count) continue;          // keep a workgroup per CU
            const bool split = nl == 4;
            size_t a, b;
            if (split) { a = std::max(f * out_bytes(3), f * out_bytes(5)); b = std::max((size_t)(f / 2) * in_bytes_of(3), f * out_bytes(4)); }
            else { a = std::max(f * in_bytes_of(4), f * out_bytes(5)); b = f * out_bytes(4); }
            a = (a + 15) & ~(size_t)15; b = (b + 15) & ~(size_t)15;
            const size_t total = a + b + 4 * 128 * 4;
            if (total > (size_t)kPilotLdsDb) continue;
            PilotChain q;
            constexpr int nw = 8;                                               // waves per workgroup, one workgroup per CU
            q.first = first; q.lds = (int)total;
            q.F = f; q.nl = nl; q.split_first = split ? 1 : 0; q.offA = 0; q.offB = (int)a; q.off_bias = (int)(a + b);
            for (int j = 0; j < nl; ++j) {
                const PilotLayer& l = L[first + j];
                // item shape per layer: items = ceil(pixels / (32 nt)) x (COUT / (32 nb)), dealt round-robin to 8 waves; waves w and w + 4 share
                // a SIMD (one workgroup per CU): the shape that leaves the busiest SIMD the fewest MFMAs per k-step, and among equals the one
                // that gives that SIMD two waves (a lone wave per SIMD exposes every LDS and L2 round trip: stamps, profiles/r03_pilot_chain.txt)
                const int px = (split && j == 0 ? f / 2 : f) * l.OH * l.OW;
                auto busiest = [&](int nt, int nb, int& waves_on_it) {
                    const int items = ((px + 32 * nt - 1) / (32 * nt)) * (l.COUT / (32 * nb));
                    int worst = 0; waves_on_it = 0;
                    for (int sd = 0; sd < 4; ++sd) {
                        int n_items = 0, n_waves = 0;
                        for (int w = sd; w < nw; w += 4) { const int mine = items > w ? (items - w + nw - 1) / nw : 0; n_items += mine; n_waves += mine > 0; }
                        if (n_items * nt * nb > worst) { worst = n_items * nt * nb; waves_on_it = n_waves; }
                    }
                    return worst;
                };
                // the better tile height (2 or 3 tiles of 32 pixels) for items of 64 output channels (items of 32 channels — twice the ring depth,
                // two waves on every SIMD — were measured in round 3: the kernel 105 k against 107 k clocks, the closed loop equal; removed in round 4, and measured once
                // more for conv7 alone, whose 64-channel items are 6 for 8 waves or 4 lone waves: chain 46.3 -> 47.5 us, for every layer 49.5; conv7 on ten single-tile
                // items of 64 channels (three per busy SIMD instead of four lone waves): 43.4 -> 46.5 us — twice the weight stream per MFMA)
                int nt = 2, best = 1 << 30, best_waves = 0;
                for (int cnt = 3; cnt >= 2; --cnt) {
                    int wv = 0;
                    const int m = busiest(cnt, 2, wv);
                    if (m < best || (m == best && wv > best_waves)) { best = m; best_waves = wv; nt = cnt; }
                }
                q.nt[j] = nt; q.nb[j] = 2; q.magic_uout[j] = pilot_magic(l.OH * l.OW); q.magic_ow[j] = pilot_magic(l.OW);
            }
            return q;
        }
    }
    return PilotChain{};
}
// Everything trs_pilot_load decides for frames of H x W, n_cap of them at most, on cu_count CUs: n_arrays = 22 (cnn_2d_speed_control / cnn_2d),
// 28 (cnn_2d_speed_as_feature) or 42 (cnn_2d_full_house, which adds dense4).  A shape the kernels cannot serve comes back as err / err_text.
inline PilotPlan pilot_plan(int H, int W, int n_cap, int cu_count, int n_arrays, const trs_pilot_tuning& T)
{
    PilotPlan P;
    P.H = H; P.W = W; P.n_cap = n_cap; P.cu_count = cu_count; P.tun = T;
    P.arch = n_arrays == 28 ? TRS_PILOT_SPD_FTR : (n_arrays == 42 ? TRS_PILOT_FULL_HOUSE : TRS_PILOT_SPD_CTL);
    P.n_layers = P.arch == TRS_PILOT_FULL_HOUSE ? 9 : 8;
    auto refuse = [&](const char* text) { P.err = TRS_ERR_LIMIT; P.err_text = text; return P; };
    int ih = H, iw = W;
    for (int i = 0; i < P.n_layers; ++i) {
        PilotLayer& l = P.L[i] = pilot_layer_geometry(i, ih, iw);
        if (l.OH < 1 || l.OW < 1) return refuse("image too small for Keras_2D_CNN");
        if (i >= 7 && (l.COUT_PAD != 128 || l.G % 16 != 0)) return refuse("dense1's shape does not suit trs_pilot_dense_kernel");   // (never for Keras_2D_CNN: 100 outputs, 16 granules per pixel of conv7's output)
        if (i < 7 && !plan_single(l, i, T)) return refuse("a convolution's weight slice does not fit LDS");   // (never for Keras_2D_CNN)
        if (i >= 3 && i < 7 && ((T.frame_layers_mask >> i) & 1)) plan_frame(l, n_cap, cu_count);   // bit i = conv(i+1) (0x78)
        if (i == 2 && T.frame5) plan_frame5(l);
        if (i < 7) { ih = l.OH; iw = l.OW; }
    }
    P.head = plan_head(P.L[0], P.L[1], T);
    P.chain = plan_chain(P.L, n_cap, cu_count, T);
    return P;
}
// which kernel a layer runs on when it is launched by itself (conv1..7); in a forward pass the fused head takes conv1 and conv2 (pilot_head_runs) and
// the chain conv(first + 1)..conv7
enum PilotKernel { kKernU8, kKernSpan1, kKernSpan2, kKernLt1, kKernLt2, kKernFrame, kKernFrame5 };
inline PilotKernel pilot_kernel_of(const PilotLayer& l)
{
    if (l.frame5 || l.frame) return l.frame5 ? kKernFrame5 : kKernFrame;
    if (l.u8in) return kKernU8;                                             // conv1 as its own layer
    if (l.res_span) return l.res_nb == 1 ? kKernSpan1 : kKernSpan2;         // conv2 unfused (24 input channels: 6 granules per pixel pair, no swizzle); conv3 where its frames do not fit LDS
    return l.res_nb == 1 ? kKernLt1 : kKernLt2;                             // the fallback of every other (layer, shape)
}
inline bool pilot_head_runs(const PilotPlan& P) { return P.head.on && !P.tun.no_fuse; }

// ---- what a call of n frames adds -------------------------------------------------------------------------------------------------
// K slices of trs_pilot_dense_kernel: whole LDS chunks, as many slices as give every CU a workgroup (groups of 32 NF frames x slices).
// NF = 2 (64 frames per workgroup share every weight fragment) where the K dimension is long enough that every workgroup still gets two
// chunks or more (240x320: 8,816 granules; at 120x160 a slice is one chunk and the kernel is launch-bound: NF = 1).
struct DenseCall { int nf, gps, KS, groups, grid, lds; };
inline DenseCall dense_call(const PilotLayer& l, int n, int cu_count, const trs_pilot_tuning& T)
{
    const int G = l.G, chunks = (G + kDenseChunk - 1) / kDenseChunk, groups2 = (n + 63) / 64, want2 = std::max(1, cu_count / groups2);
    DenseCall d{};
    d.nf = (n >= 64 && (chunks + want2 - 1) / want2 >= 2 && T.dense != 2) ? 2 : 1;   // tuning: dense = 2 keeps 32 frames per workgroup (A/B)
    d.groups = (n + 32 * d.nf - 1) / (32 * d.nf);
    const int want = T.ksplit > 0 ? T.ksplit : std::max(1, cu_count / d.groups);
    d.gps = std::max(1, (chunks + want - 1) / want) * kDenseChunk;          // whole chunks per slice
    d.KS = (G + d.gps - 1) / d.gps;
    d.grid = d.groups * ((d.KS + 7) / 8) * 8; d.lds = d.nf * kDenseLds;
    return d;
}
// the fused head: rolling bands when there are enough (frame, part) streams for every CU (a small batch keeps one band per workgroup: more parallelism)
struct HeadCall { int roll, grid; };
inline HeadCall head_call(const PilotPlan& P, int n)
{
    const int parts = std::max(1, P.head.wsplit), roll = (P.tun.fuse_roll && n * parts >= P.cu_count && P.head.bands > 1) ? 1 : 0;
    return HeadCall{roll, roll ? std::min(n * parts, P.cu_count) : std::max(1, std::min(n * P.head.bands * parts, P.cu_count))};
}
// one persistent workgroup per CU walks the units (frame5) or the groups of F units (frame); the chain takes F frames per workgroup
inline int frame5_grid(const PilotLayer& l, int n, int cu_count) { return std::min(n * l.frame5_bands, cu_count); }
inline int frame_grid(const PilotLayer& l, int n, int cu_count) { return std::min((n * l.frame_bands + l.frame_f - 1) / l.frame_f, cu_count); }
inline int chain_grid(const PilotChain& c, int n) { return (n + c.F - 1) / c.F; }
inline int single_grid_x(const PilotLayer& l, int n, int cu_count)            // the single-layer kernels: grid (x, res_ysplit)
{
    const int waves = l.res_block / 64, ntiles = (n * l.OH * l.OW + 31) / 32;
    return std::max(1, std::min((ntiles + waves - 1) / waves, cu_count * l.res_wg_per_cu));
}

// ---- weight packing ---------------------------------------------------------------------------------------------------------------
// binary32 -> binary16, round to nearest even; weights beyond binary16's range saturate (|w| > 65504 does not occur in a trained network)
inline unsigned short host_f2h(float f)
{
    uint32_t x; std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (unsigned short)(sign | 0x7E00u | ((a >> 13) & 0x1FFu));   // NaN stays NaN
    if (a >= 0x477FE000u) return (unsigned short)(sign | 0x7BFFu);                          // 65504 and beyond
    const bool sub = a < 0x38800000u;                                       // below 2^-14: a binary16 subnormal, in units of 2^-24
    const int shift = sub ? 126 - (int)(a >> 23) : 13;
    if (shift > 24) return (unsigned short)sign;
    const uint32_t m = sub ? (a & 0x7FFFFFu) | 0x800000u : a - 0x38000000u, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    const uint32_t r = (m >> shift) + ((rem > half || (rem == half && ((m >> shift) & 1u))) ? 1u : 0u);
    return (unsigned short)(sign | r);
}
// binary16 -> binary32, exact (the debug getter's; packing needs host_f2h only)
inline float host_h2f(unsigned short u)
{
    const uint32_t sign = (uint32_t)(u & 0x8000u) << 16, e = (u >> 10) & 0x1Fu, m = u & 0x3FFu;
    uint32_t x;
    if (e == 0x1Fu) x = sign | 0x7F800000u | (m << 13);                     // infinity, NaN
    else if (e) x = sign | ((e + 112u) << 23) | (m << 13);
    else {                                                                  // zero or a subnormal: m x 2^-24
        const float f = (float)m * (1.0f / 16777216.0f);
        std::memcpy(&x, &f, 4); x |= sign;
    }
    float f; std::memcpy(&f, &x, 4);
    return f;
}
// w: granules [G_pad][COUT_PAD][8] of fp16; goff: [G_pad] byte offset of granule g relative to the output pixel's input base; bias: [COUT_PAD]
struct PackedLayer { std::vector<unsigned short> w; std::vector<int> goff; std::vector<float> bias; };
// K: the Keras kernel [KH][KW][CIN][COUT] (dense: [CIN][COUT]), B: its bias [COUT]
inline PackedLayer pack_layer(const PilotLayer& l, const float* K, const float* B)
{
    PackedLayer p{std::vector<unsigned short>((size_t)l.G_pad * l.COUT_PAD * 8, 0), std::vector<int>(l.G_pad, 0), std::vector<float>(l.COUT_PAD, 0.0f)};
    for (int g = 0; g < l.G; ++g) {
        if (l.u8in) {
            const int kh = g >> 1, half = g & 1;
            p.goff[g] = kh * l.IW * 3 + 8 * half;
            for (int j = 0; j < 8; ++j) {
                const int f = 8 * half + j;                       // byte f of the 16-byte row window = (kw, c), 15 is padding
                if (f >= 15) continue;
                const int kw = f / 3, ch = f % 3;
                for (int co = 0; co < l.COUT; ++co)
                    p.w[((size_t)g * l.COUT_PAD + co) * 8 + j] = host_f2h(K[((kh * l.KW + kw) * l.CIN + ch) * l.COUT + co] * (256.0f / 255.0f));   // x 2^-8 in the epilogue (kConv1Scale)
            }
        } else {
            const int kh = g / l.run_pad, gi = g % l.run_pad;             // granule gi of kernel row kh
            p.goff[g] = (kh * l.IW * l.CIN + gi * 8) * 2;
            if (gi >= l.run) continue;                                    // run padding: next pixel's bytes x zero weights
            const int c8n = l.CIN / 8, kw = gi / c8n, c8 = gi % c8n;
            for (int j = 0; j < 8; ++j)
                for (int co = 0; co < l.COUT; ++co)
                    p.w[((size_t)g * l.COUT_PAD + co) * 8 + j] = host_f2h(K[((size_t)(kh * l.KW + kw) * l.CIN + c8 * 8 + j) * l.COUT + co]);
        }
    }
    for (int g = l.G; g < l.G_pad; ++g) p.goff[g] = p.goff[l.G - 1];       // padding granule: valid address, zero weights
    for (int co = 0; co < l.COUT; ++co) p.bias[co] = B[co];
    return p;
}
// The band kernel reads conv1 columns by parity: slot sl of a kernel row of conv2 (16 granules) holds granule kw * 3 + c8 of the row in
// the order even conv1 columns (kw 0, 2, 4), then the odd (1, 3), then the padding granule 15.
inline int conv2_parity_src(int sl) { return sl < 9 ? (2 * (sl / 3)) * 3 + sl % 3 : (sl < 15 ? (2 * ((sl - 9) / 3) + 1) * 3 + (sl - 9) % 3 : 15); }
inline std::vector<unsigned short> conv2_parity_order(const PilotLayer& l1, const std::vector<unsigned short>& w)
{
    const size_t row = (size_t)l1.COUT_PAD * 8;                           // values per granule slot
    std::vector<unsigned short> perm(w.size());
    for (int sl = 0; sl < 5 * 16; ++sl) std::copy_n(&w[(size_t)(sl / 16 * 16 + conv2_parity_src(sl % 16)) * row], row, &perm[(size_t)sl * row]);
    return perm;
}
// Can conv1 leave binary16's range?  Its inputs are pixels / 256 <= 1, so |output| <= |bias| + sum |w| (x 256 / 255 and the binary16 rounding of the
// weights: 1.01 covers both).  Below 65504 for every output channel the fused head's conv1 epilogue needs no saturation step.
inline int conv1_bounded(const PilotLayer& l0, const float* K0, const float* B0)
{
    for (int co = 0; co < l0.COUT; ++co) {
        double sum = std::fabs((double)B0[co]);
        for (int k = 0; k < l0.KH * l0.KW * l0.CIN; ++k) sum += std::fabs((double)K0[(size_t)k * l0.COUT + co]) * 1.01;
        if (!(sum < 60000.0)) return 0;                                   // (a NaN weight: not bounded)
    }
    return 1;
}

// ---- the small fp32 weights of the tail kernels: one blob per loaded model ----------------------------------------------------------
// Slot XO_x of the blob = Keras array x, whole and in Keras's [IN][OUT] layout, except the two that are the rows of dense1 / dense4 BEHIND the flatten
// (XO_W1Y, XO_W4Y: the rows the matrix cores do not take).  F1..3 = feature1..3, C1..3 = current_spd_1..3, W2..B4 = dense2, dense3 and the first head's
// output, W5..B7 = dense5, dense6, out_steering.  22 arrays fill W2..B4 only (trs_pilot_tail_kernel reads nothing else), 28 all up to B4, 42 every slot.
enum { XO_F1W, XO_F1B, XO_F2W, XO_F2B, XO_F3W, XO_F3B, XO_W1Y, XO_W2, XO_B2, XO_W3, XO_B3, XO_W4, XO_B4,
       XO_C1W, XO_C1B, XO_C2W, XO_C2B, XO_C3W, XO_C3B, XO_W4Y, XO_W5, XO_B5, XO_W6, XO_B6, XO_W7, XO_B7, XO_COUNT };
struct TailLayout {
    int xo[32] = {};                       // offset (floats) of slot XO_x in the blob; 0 for a slot the architecture does not have
    int f1 = 0, f2 = 0, f3 = 0;            // widths of the small input branches: 4, 8, 16 (cnn_2d_speed_as_feature) or 16, 32, 64 (cnn_2d_full_house); 0: none
};
struct TailBlob : TailLayout { std::vector<float> data; };
// arr: the Keras arrays in trs_pilot_load's order, each exactly its Keras size (dense1 is [F + f3][100], dense4 [F + 2 f3][100], F = P.L[7].CIN)
inline TailBlob pack_tail_blob(const PilotPlan& P, const float* const* arr)
{
    TailBlob t;
    const size_t F = (size_t)P.L[7].CIN;
    const int nz = P.arch == TRS_PILOT_FULL_HOUSE ? 1 : 2;                // outputs of the first head
    auto put = [&](int slot, const float* src, size_t n) { t.xo[slot] = (int)t.data.size(); t.data.insert(t.data.end(), src, src + n); };
    // a branch 1 -> f1 -> f2 -> f3 from six consecutive arrays into six consecutive slots
    auto branch = [&](int slot, int a) {
        const size_t n[6] = {(size_t)t.f1, (size_t)t.f1, (size_t)t.f1 * t.f2, (size_t)t.f2, (size_t)t.f2 * t.f3, (size_t)t.f3};
        for (int j = 0; j < 6; ++j) put(slot + j, arr[a + j], n[j]);
    };
    // dense(a) -> dense(a + 2) -> an output of nout: 100 -> 50 -> 25 -> nout
    auto head = [&](int slot, int a, int nout) {
        const size_t n[6] = {100 * 50, 50, 50 * 25, 25, (size_t)25 * nout, (size_t)nout};
        for (int j = 0; j < 6; ++j) put(slot + j, arr[a + j], n[j]);
    };
    if (P.arch != TRS_PILOT_SPD_CTL) {
        t.f1 = P.arch == TRS_PILOT_SPD_FTR ? 4 : 16; t.f2 = 2 * t.f1; t.f3 = 4 * t.f1;
        branch(XO_F1W, 22);
        put(XO_W1Y, arr[14] + F * 100, (size_t)t.f3 * 100);               // dense1's rows behind the flatten
    }
    head(XO_W2, 16, nz);
    if (P.arch == TRS_PILOT_FULL_HOUSE) {
        branch(XO_C1W, 28);
        put(XO_W4Y, arr[34] + F * 100, (size_t)2 * t.f3 * 100);           // dense4's rows for [feature3 | current_spd_3]
        head(XO_W5, 36, 1);
    }
    return t;
}

}  // namespace trsim
