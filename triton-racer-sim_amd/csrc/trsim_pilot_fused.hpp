// trsim_pilot_fused.hpp — the pilot's fused convolution kernels: a 3x3 layer with its input frames in LDS (trs_conv_frame_kernel), conv4 .. conv7 in one launch
// (trs_conv_chain_kernel), conv3 with its input frames in LDS (trs_conv_frame5_kernel) and conv1 -> conv2 with conv1's activation in LDS (trs_conv12_band_kernel).
// Included by trsim_pilot.hip inside its anonymous namespace, behind trsim_pilot_mma.hpp; the parameter blocks are trsim_pilot_pass.hpp's.

#ifndef TRS_FRAME_STAMPS
#define TRS_FRAME_STAMPS 0   /* diagnostic build, never shipped: workgroup 7 prints the s_memtime ticks of its staging, work and waits */
#endif
#ifndef TRS_FRAME_R
#define TRS_FRAME_R 4   /* weight ring depth of trs_conv_frame_kernel in k-steps */
#endif
#ifndef TRS_FRAME_ABLATE
#define TRS_FRAME_ABLATE 0   /* timing-only diagnostic builds of trs_conv_frame_kernel, never shipped: 1 = no weight refills, 3 = no stores, 4 = no staging */
#endif

// Round 4: persistent and double-buffered, like trs_conv_frame5_kernel.  Until then a workgroup staged its F units, computed them and ended; its
// ~150-200 registers allow one 8-wave workgroup per CU, so nothing ran beside the staging: a timing-only build without it (-DTRS_FRAME_ABLATE=4)
// put it at 16-25 % of the 240x320 layers (conv4 49.1 -> 36.8 us, conv5 39.2 -> 29.8, conv6 58.9 -> 49.6, conv7 99.4 -> 83.7 per 512 frames).
// Now one workgroup per CU walks its groups of F units: COMPUTE waves work on group i from one LDS buffer while LOADERS waves run the LDS-DMA
// of group i + 1 into the other; one barrier per group.  The weights come by buffer load (one lane offset + a scalar per k-step: no 64-bit
// address per ring slot — ~60 registers less, which is what lets 12 waves of <= 168 registers share the CU).
template <int NT, int NB, int HALF, int R, int COMPUTE, int LOADERS>
__global__ __launch_bounds__(64 * (COMPUTE + LOADERS), 1) void trs_conv_frame_kernel(const FrameConvParams p)
{
    constexpr int nwaves = COMPUTE + LOADERS, BLOCK = 64 * nwaves;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int n_units = p.N * p.bands, n_groups = (n_units + p.F - 1) / p.F;
    const int upix = p.ihb * p.IW, uout = p.ohb * p.OW;                     // input pixels staged / output pixel slots per unit
    const unsigned buf_bytes = (unsigned)((p.F * upix) << p.cgs) * 16u;     // one group of units in LDS
    const unsigned lds_base = (unsigned)(uintptr_t)psmem;
    // staging of group g into the buffer at byte offset `off` by waves w0 .. w0 + nw - 1.  A unit's input rows are whole rows of one frame: ONE
    // contiguous run of upix x cg granules in memory (stage_run; what a last band asks for below its frame is clamped into the activation)
    const int last_gran = (int)(((size_t)p.N * p.IH * p.IW) << p.cgs) - 1;
    auto stage = [&](int g, unsigned off, int w0, int nw) {
        const int u0 = g * p.F, nu = min(p.F, n_units - u0);
        const int total = upix << p.cgs;                                    // granule slots of one unit
        for (int ul = 0; ul < nu && TRS_FRAME_ABLATE != 4; ++ul) {
            const int u = u0 + ul, f = u / p.bands, band = u - f * p.bands;  // (wave-uniform: scalar unit)
            const int base = ((f * p.IH + band * p.ohb) * p.IW) << p.cgs;     // first granule of the unit in the activation (< 2^31: in_bytes fits an int)
            stage_run(p.in + base, total, last_gran - base, ul * upix, p.cgs, lds_base + off + (unsigned)(ul * total) * 16u, wave - w0, nw, lane);
        }
    };
    float* lb = reinterpret_cast<float*>(psmem + 2 * (size_t)buf_bytes);    // the bias behind the two buffers
    const float4* lbias = reinterpret_cast<const float4*>(lb);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u4v*>(p.w), 0, 9 * p.cg * p.COUT_PAD * 16, 0x00020000);   // [9 taps x cg granules][COUT_PAD] granules
    PhaseStamps<TRS_FRAME_STAMPS != 0> stamps;
    int g = blockIdx.x;
    if (g < n_groups) stage(g, 0u, 0, nwaves);                              // the first group: all waves
    for (int i = tid; i < p.COUT_PAD; i += BLOCK) lb[i] = p.bias[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamps.mark(stamps.kStaging);
    const int n_cgrp = p.COUT_PAD / (NB * 32);
    for (int it = 0; g < n_groups; ++it, g += gridDim.x) {
        const unsigned cur = (it & 1) ? buf_bytes : 0u;
        if (wave >= COMPUTE) {                                              // loaders: the next group into the other buffer
            if (g + (int)gridDim.x < n_groups) stage(g + (int)gridDim.x, buf_bytes - cur, COMPUTE, LOADERS);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            const int u0 = g * p.F, nu = min(p.F, n_units - u0);
            int m_wg = nu * uout;                                           // output pixel slots of this group
            if (p.F == 1 && p.bands > 1) {                                  // one unit: a short last band has no tiles for the rows below the frame
                const int band = u0 % p.bands;
                m_wg = min(p.ohb, p.OH - band * p.ohb) * p.OW;
            }
            const int n_tiles = (m_wg + NT * 32 - 1) / (NT * 32);
            for (int item = wave; item < n_tiles * n_cgrp; item += COMPUTE) {
                const int cgrp = item / n_tiles, tile = item - cgrp * n_tiles;
                const int cbase = cgrp * NB * 32;
                int lbase[NT];                                              // linear LDS pixel index of each of this lane's windows
                long long obase[NT];                                        // output pixel index in the layer's activation, -1 = no such pixel
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int m = tile * NT * 32 + nt * 32 + r, mc = min(m, m_wg - 1);
                    const int ul = (int)__umulhi((unsigned)mc, p.magic_uout), rem = mc - ul * uout, oyl = (int)__umulhi((unsigned)rem, p.magic_ow), ox = rem - oyl * p.OW;
                    const int u = u0 + ul, f = p.magic_bands ? (int)__umulhi((unsigned)u, p.magic_bands) : u, oy = (u - f * p.bands) * p.ohb + oyl;   // (magic 0: one band per frame)
                    lbase[nt] = (ul * p.ihb + oyl) * p.IW + ox;
                    obase[nt] = (m < m_wg && oy < p.OH) ? ((long long)f * p.OH + oy) * p.OW + ox : -1;
                }
                // a 3x3 item of the group's image (conv3x3_item: the weights by buffer load through a register ring, the K loop one basic block)
                f32x16 acc[NT][NB];
                conv3x3_item<HALF, R, TRS_FRAME_ABLATE == 1 ? 1 : 0>(acc, lds_base + cur, p.IW, rw, p.COUT_PAD, lbias, cbase, lbase, r, h);
                // epilogue (block_groups): lane h = 0 stores channel groups 0, 1 of a block, lane h = 1 groups 2, 3 — whole 16-byte groups
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    unsigned short* o = p.out + (size_t)(obase[nt] < 0 ? 0 : obase[nt]) * p.COUT + cbase;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        u4v g0, g1;
                        block_groups(acc[nt][nb], g0, g1);
#if TRS_FRAME_ABLATE == 3
                        asm volatile("" :: "v"(g0), "v"(g1)); (void)o;
#else
                        if (obase[nt] >= 0) {
                            *reinterpret_cast<u4v*>(o + nb * 32 + 16 * h) = g0;       // channels nb*32 + 16h .. + 7
                            *reinterpret_cast<u4v*>(o + nb * 32 + 16 * h + 8) = g1;   // ... + 8 .. + 15
                        }
#endif
                    }
                }
            }
        }
        stamps.mark(stamps.kWork);
        __syncthreads();                                                    // the next group is in LDS, this one has been read
        stamps.mark(stamps.kWait);
    }
#if TRS_FRAME_STAMPS
    if (blockIdx.x == 7 && lane == 0 && (wave == 0 || wave == COMPUTE - 1 || wave == COMPUTE))
        printf("frame kernel (cg %d, COUT %d, bands %d, F %d, %d groups), workgroup 7, wave %d [ticks]: first staging %lld | groups: work %lld, wait at the barrier %lld\n",
               p.cg, p.COUT, p.bands, p.F, n_groups, wave, stamps.ticks[0], stamps.ticks[1], stamps.ticks[2]);
#endif
}

// ---- conv4 .. conv7 in ONE launch: a frame's activations never leave LDS (round 2) ---------------------------------------------
// The time line of a workgroup of this loop (profiles/r02_pilot_dense.txt) shows ~3 us from dispatch to the first data in LDS and
// ~2.3 us from the last store to the end of the launch; the four 3x3 layers paid that four times over for 4-10 us of work each,
// plus a global round trip of every activation.  At 120x160 the four layers of F = 4 frames fit LDS together:
//   region A (76.8 KB): conv4's output -> (conv5 reads) -> conv6's output -> (conv7 reads)
//   region B (53.2 KB): conv4's input, two frames at a time -> conv5's output -> (conv6 reads)
// conv4 runs in two passes of two frames (its input is the largest tensor of the chain: 26 KB per frame); conv7 stores to global.
// A layer is trs_conv_frame_kernel's item (conv3x3_item: 2 x 32 pixels x 2 x 32 channels per wave, weights straight from L2
// through a register ring, the K loop one basic block); its epilogue writes the next layer's LDS image — 16-byte granules in the
// same XOR-swizzled slots the staging DMA would have produced.  Layers are separated by a workgroup barrier only.
#ifndef TRS_CHAIN_ABLATE
#define TRS_CHAIN_ABLATE 0   /* timing-only diagnostic builds of the chain's layers, never shipped: 1 = no weight refills, 2 = one LDS pixel read per item, 3 = no MFMA */
#endif
// One layer of the chain.  A wave item = NT x 32 pixels x NB x 32 output channels; the weight ring is R k-steps deep (R x NB granules per
// lane: NB = 1 takes twice the depth for the same registers and the same lead time in MFMA clocks).
template <int HALF, int R, int NT, int NB>
__device__ __forceinline__ void chain_layer(const ChainLayer& L, const u4v* lin, const float* lbias_f, int nu, u4v* lout, int cgs_out, int out_pix0,
                                            unsigned short* gout, int wave, int nwaves, int lane)
{
    const int r = lane & 31, h = lane >> 5;
    const int uout = L.OH * L.OW, m_wg = nu * uout;
    const int n_tiles = (m_wg + NT * 32 - 1) / (NT * 32), n_cgrp = L.COUT / (NB * 32);
    const float4* lbias = reinterpret_cast<const float4*>(lbias_f);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u4v*>(L.w), 0, 9 * L.cg * L.COUT * 16, 0x00020000);   // [9 taps x cg granules][COUT] granules
    const unsigned lin_b = (unsigned)(uintptr_t)lin;                                // LDS byte address of the layer's input image
    for (int item = wave; item < n_tiles * n_cgrp; item += nwaves) {
        const int cgrp = item / n_tiles, tile = item - cgrp * n_tiles;
        const int cbase = cgrp * NB * 32;
        int lbase[NT], mo[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int m = tile * NT * 32 + nt * 32 + r, mc = min(m, m_wg - 1);
            const int ul = (int)__umulhi((unsigned)mc, L.magic_uout), rem = mc - ul * uout, oy = (int)__umulhi((unsigned)rem, L.magic_ow), ox = rem - oy * L.OW;
            lbase[nt] = (ul * L.IH + oy) * L.IW + ox;
            mo[nt] = m < m_wg ? m : -1;
        }
        f32x16 acc[NT][NB];
        conv3x3_item<HALF, R, TRS_CHAIN_ABLATE>(acc, lin_b, L.IW, rw, L.COUT, lbias, cbase, lbase, r, h);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                u4v g0, g1;
                block_groups(acc[nt][nb], g0, g1);                          // lane h = 0: channel groups 0, 1 of this block, lane h = 1: groups 2, 3 (whole 16-byte groups)
                if (mo[nt] >= 0) {
                    if (lout) {                                               // the next layer's image: pixel slot, granule ^ swizzle
                        const int po = out_pix0 + mo[nt], q0 = (cbase + nb * 32 + 16 * h) >> 3, sw = frame_swz(po, cgs_out);
                        lout[(po << cgs_out) + (q0 ^ sw)] = g0;
                        lout[(po << cgs_out) + ((q0 + 1) ^ sw)] = g1;
                    } else {
                        unsigned short* o = gout + (size_t)mo[nt] * L.COUT + cbase + nb * 32 + 16 * h;
                        *reinterpret_cast<u4v*>(o) = g0;
                        *reinterpret_cast<u4v*>(o + 8) = g1;
                    }
                }
            }
        }
    }
}
#ifndef TRS_CHAIN_R
#define TRS_CHAIN_R 4   /* weight ring depth of the chain's layers in k-steps at NB = 2 (twice that at NB = 1) */
#endif
// (tile height, channel blocks) of a layer -> its instantiation
template <int HALF>
__device__ __forceinline__ void chain_layer_any(const ChainLayer& L, const u4v* lin, const float* lbias_f, int nu, u4v* lout, int cgs_out, int out_pix0,
                                                unsigned short* gout, int wave, int nwaves, int lane)
{
    if (L.nt == 3) chain_layer<HALF, TRS_CHAIN_R, 3, 2>(L, lin, lbias_f, nu, lout, cgs_out, out_pix0, gout, wave, nwaves, lane);
    else chain_layer<HALF, TRS_CHAIN_R, 2, 2>(L, lin, lbias_f, nu, lout, cgs_out, out_pix0, gout, wave, nwaves, lane);
}
template <int BLOCK>
__global__ __launch_bounds__(BLOCK, 2) void trs_conv_chain_kernel(const ChainParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int nwaves = BLOCK / 64;
    const int u0 = blockIdx.x * p.F, nu = min(p.F, p.N - u0);
    float* const lb = reinterpret_cast<float*>(psmem + p.off_bias);         // [layer][128]
    for (int li = 0; li < p.nl; ++li)
        for (int i = tid; i < p.L[li].COUT; i += BLOCK) lb[li * 128 + i] = p.L[li].bias[i];
    u4v* const A = reinterpret_cast<u4v*>(psmem + p.offA);
    u4v* const B = reinterpret_cast<u4v*>(psmem + p.offB);
    const unsigned lds0 = (unsigned)(uintptr_t)psmem;
    auto stage = [&](const ChainLayer& L, int fa, int cnt, unsigned lds_byte) {   // frames fa .. fa + cnt - 1 of L's input, whole and contiguous
        const int upix = L.IH * L.IW, total = (cnt * upix) << L.cgs;
        stage_run(p.in + ((size_t)fa * upix << L.cgs), total, total - 1, 0, L.cgs, lds_byte, wave, nwaves, lane);
    };
    int li = 0;
    const u4v* cur = A;
    if (p.split_first) {
        const ChainLayer& L0 = p.L[0];
        const int per = p.F / 2;
        for (int pass = 0; pass < 2; ++pass) {
            const int cnt = min(per, nu - per * pass);                      // workgroup-uniform
            if (cnt > 0) stage(L0, u0 + per * pass, cnt, lds0 + p.offB);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (cnt > 0) {
                chain_layer_any<4>(L0, B, lb, cnt, A, p.L[1].cgs, per * pass * L0.OH * L0.OW, nullptr, wave, nwaves, lane);
            }
            __syncthreads();
        }
        li = 1;
    } else {
        stage(p.L[0], u0, nu, lds0 + p.offA);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    for (; li < p.nl - 1; ++li) {
        const ChainLayer& L = p.L[li];
        u4v* const nxt = cur == A ? B : A;
        chain_layer_any<4>(L, cur, lb + li * 128, nu, nxt, p.L[li + 1].cgs, 0, nullptr, wave, nwaves, lane);
        __syncthreads();
        cur = nxt;
    }
    {
        const ChainLayer& L = p.L[p.nl - 1];
        chain_layer_any<8>(L, cur, lb + (p.nl - 1) * 128, nu, nullptr, 0, 0, p.out + (size_t)u0 * L.OH * L.OW * L.COUT, wave, nwaves, lane);
    }
}

// (Round 5 rebuilt this chain on v_mfma_f32_16x16x32_f16 with a conflict-free LDS image — two planes of channel granules, host tables that fill 16-pixel blocks by
// residue class: bank conflicts 46 % -> 9.5 % of the LDS cycles, MFMA cycles -15 % — and it was 7-14 % SLOWER on every box: the K loops are bound by the instructions
// around the MFMAs, and a 16x16x32 MFMA takes twice the issue slots per FLOP.  Removed again; profiles/r05_pilot_chain16.txt has the numbers and the stamps.)
// ---- conv3 with its input frames in LDS (round 2) -----------------------------------------------------------------------------
// conv3 (5x5 stride 2, 32 -> 64 channels) on the span kernel below reads three 1 KB fragments from LDS per two MFMAs (its weights
// live in LDS: 192 B/clk per CU at full MFMA rate against the 128 the LDS delivers) — 43 us per 1024 frames.  This is the frame
// kernel's scheme instead: F = 2 input frames (64 KB each) in LDS by LDS-DMA, weights straight from L2 through a register ring,
// 2 x 32 pixels x 2 x 32 channels per wave, the 50 k-steps (25 taps x 2 halves of the 32 input channels) one basic block.
// Stride 2 changes the LDS image: a row is stored as its even columns, then its odd columns, so the windows of consecutive
// output pixels are consecutive 64-byte slots for every tap; granule g of slot s sits at g ^ ((s >> 2) & 3) — 16 consecutive
// slots of one logical granule cover all 64 banks.
#ifndef TRS_F5_R
#define TRS_F5_R 4   /* weight ring depth of trs_conv_frame5_kernel in k-steps */
#endif
#ifndef TRS_F5_NB
#define TRS_F5_NB 2        /* 32-channel blocks per wave item */
#endif
#ifndef TRS_F5_STAMPS
#define TRS_F5_STAMPS 0   /* diagnostic build, never shipped: workgroup 7 prints the s_memtime ticks of its first staging, its work and its waits */
#endif

// Round 4: the workgroup is persistent and double-buffered.  Until then a 4-wave workgroup took ONE unit (two workgroups per CU, "one stages
// while the other computes") — but all workgroups of a launch start together, so both of a CU staged at the same time and then computed at the
// same time: stamps (-DTRS_F5_STAMPS=1) showed 10-12 k clocks of staging — 512 workgroups pulling 64 KB each at once: the fabric's ~6.5 TB/s —
// in front of 10-11 k clocks of K loops, twice over for the 1024 frames.  Now one 8-wave workgroup per CU walks its units: waves 0..3 compute unit i
// (one NT x 2 item each at 120x160) from one LDS buffer while waves 4..7 run the LDS-DMA of unit i + 1 into the other; one barrier per unit.
// conv3 33.5 -> 31.1 us per 1024 frames.  What is left (stamps of the persistent form, profiles/r04_pilot_frame5.txt): a unit's K loops take 10.5-11.6 k
// s_memtime ticks for 200 MFMAs per wave (5.6 k at the MFMA rate: ONE compute wave per SIMD keeps its pipe ~55 % busy; two waves per SIMD of the old form
// kept it full, but staged and computed in lockstep).  Timing-only builds: no weight refills -8 %, refills always from L1 -7 %, no pixel reads -2 % —
// neither operand stream is what holds a lone wave back.  Measured and not kept: 8 compute waves on 32-channel items (NB = 1: twice the LDS
// traffic) 32.4 us; 8 compute waves on the four NB = 2 items (half of them idle) 31.4; weight rings 8 and 12 k-steps deep (possible since the
// weights come by buffer load: 138 registers instead of 234) 32.3 / 32.5.
template <int NT, int NB, int R, int BLOCK, int COMPUTE>
__global__ __launch_bounds__(BLOCK, 1) void trs_conv_frame5_kernel(const Frame5Params p)
{
    constexpr int KW = 5, kCompute = COMPUTE;                               // waves 0 .. COMPUTE - 1 compute, the others stage
    const int COUT = p.COUT;                                                // 64 (the host checks)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nwaves = BLOCK / 64;
    static_assert(nwaves > kCompute, "loader waves");
    const int r = lane & 31, h = lane >> 5;
    const int n_units = p.N * p.bands;
    const int upix = p.ihb * p.IW;                                          // input pixels staged per unit
    const unsigned buf_bytes = (unsigned)upix * 64u;                        // one unit in LDS (a multiple of 64)
    const unsigned lds_base = (unsigned)(uintptr_t)psmem;
    PhaseStamps<TRS_F5_STAMPS != 0> stamps;
    // staging of unit u into the buffer at byte offset `off` by waves w0 .. w0 + nw - 1: slot sl = 4 * lpix + q holds granule q ^ ((lpix >> 2) & 3) of the
    // pixel that lives in slot lpix
    auto stage = [&](int u, unsigned off, int w0, int nw) {
        const int total = upix * 4;
        const int f = u / p.bands, band = u - f * p.bands;
        for (int s0 = (wave - w0) * 64; s0 < total; s0 += nw * 64) {
            const int sl = s0 + lane;
            if (sl < total) {
                const int lpix = sl >> 2, g = (sl & 3) ^ ((lpix >> 2) & 3);
                const int iyl = lpix / p.IW, sx = lpix - iyl * p.IW;
                const int col = sx < p.ev ? 2 * sx : 2 * (sx - p.ev) + 1;
                const int iy = min(2 * band * p.ohb + iyl, p.IH - 1);         // (rows below the frame are never read by a valid pixel)
                const size_t gpix = ((size_t)f * p.IH + iy) * p.IW + col;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(p.in + gpix * 4 + g),
                                                 (__attribute__((address_space(3))) void*)(uintptr_t)(lds_base + off + s0 * 16), 16, 0, 0);
            }
        }
    };
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<u4v*>(p.w), 0, 100 * COUT * 16, 0x00020000);   // [25 taps x 4 granules][COUT] granules
    const int wvoff = (h * COUT + r) * 16;
    float* lb = reinterpret_cast<float*>(psmem + 2 * (size_t)buf_bytes);
    const float4* lbias = reinterpret_cast<const float4*>(lb);
    int u = blockIdx.x;
    if (u < n_units) stage(u, 0u, 0, nwaves);                               // the first unit: all waves
    for (int i = tid; i < COUT; i += BLOCK) lb[i] = p.bias[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamps.mark(stamps.kStaging);
    for (int it = 0; u < n_units; ++it, u += gridDim.x) {
        const unsigned cur = (it & 1) ? buf_bytes : 0u;
        if (wave >= kCompute) {                                             // loaders: the next unit into the other buffer
            if (u + (int)gridDim.x < n_units) stage(u + (int)gridDim.x, buf_bytes - cur, kCompute, nwaves - kCompute);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            const int f = u / p.bands, band = u - f * p.bands;
            const int m_wg = min(p.ohb, p.OH - band * p.ohb) * p.OW;         // a short last band has no tiles for the rows below the frame
            const int n_tiles = (m_wg + NT * 32 - 1) / (NT * 32), n_cgrp = COUT / (NB * 32);
            for (int it2 = wave; it2 < n_tiles * n_cgrp; it2 += kCompute) {
                const int cgrp = it2 / n_tiles, item = it2 - cgrp * n_tiles, cbase = cgrp * NB * 32;   // (the waves of one SIMD take different tiles where they can)
                int lbase[NT];
                long long mo[NT];                                           // output pixel index in the layer's activation, -1 = no such pixel
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int m = item * NT * 32 + nt * 32 + r, mc = min(m, m_wg - 1);
                    const int oyl = (int)__umulhi((unsigned)mc, p.magic_ow), ox = mc - oyl * p.OW;
                    const int oy = band * p.ohb + oyl;
                    lbase[nt] = 2 * oyl * p.IW + ox;                        // slot of input pixel (2 oyl, 2 ox) of the unit: even plane, position ox
                    mo[nt] = m < m_wg ? ((long long)f * p.OH + oy) * p.OW + ox : -1;
                }
                // weight granule (2 k + h, cout cbase + nb*32 + r) of k-step k for ring_k_loop
                int wso = cbase * 16;                                       // the k-step part of the offset: one scalar that runs with the loads
                auto wload = [&](int nb) { return __builtin_bit_cast(u4v, __builtin_amdgcn_raw_buffer_load_b128(rw, wvoff + nb * 512, wso, 0)); };
                auto wnext = [&]() { wso += 2 * COUT * 16; asm volatile("" : "+s"(wso)); };
                unsigned tapb[NT];                                          // (the swizzled address once per tap, ^ 32 for its second k-step)
                auto pixels = [&](int k, h16x8 (&x)[NT]) {                  // k is a compile-time constant after unrolling
                    const int tap = k / 2, j = k % 2;
                    const int kh = tap / KW, kw = tap % KW;
                    const int tap_off = kh * p.IW + ((kw & 1) ? p.ev : 0) + (kw >> 1);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        if (j == 0) {
                            const int pix = lbase[nt] + tap_off;
                            tapb[nt] = lds_base + cur + (unsigned)((pix * 4 + (h ^ ((pix >> 2) & 3))) << 4);
                        }
                        x[nt] = __builtin_bit_cast(h16x8, *(lds_u4vp)(uintptr_t)(tapb[nt] ^ (unsigned)(32 * j)));
                    }
                };
                f32x16 acc[NT][NB];
                ring_k_loop<50, R, 0>(acc, lbias, cbase, h, wload, wnext, pixels);   // 25 taps x 2 halves of the 32 input channels
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    unsigned short* o = p.out + (size_t)(mo[nt] < 0 ? 0 : mo[nt]) * COUT + cbase;
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        u4v g0, g1;
                        block_groups(acc[nt][nb], g0, g1);                // lane h = 0: channel groups 0, 1 of this block, lane h = 1: groups 2, 3 (whole 16-byte groups)
                        if (mo[nt] >= 0) {
                            *reinterpret_cast<u4v*>(o + nb * 32 + 16 * h) = g0;
                            *reinterpret_cast<u4v*>(o + nb * 32 + 16 * h + 8) = g1;
                        }
                    }
                }
            }
        }
        stamps.mark(stamps.kWork);
        __syncthreads();                                                    // the next unit is in LDS, this one has been read
        stamps.mark(stamps.kWait);
    }
#if TRS_F5_STAMPS
    if (blockIdx.x == 7 && lane == 0 && (wave == 0 || wave == kCompute - 1 || wave == kCompute))
        printf("frame5, workgroup 7, wave %d [clocks]: first staging %lld | units: work %lld, wait at the barrier %lld\n", wave, stamps.ticks[0], stamps.ticks[1], stamps.ticks[2]);
#endif
}

// conv1 -> conv2 fused: conv1's activation (217 KB per 120x160 frame, the largest tensor of the network: 222 MB per 1024
// frames, written once and read once) never leaves the CU.  A workgroup takes a band of R2 conv2 output rows of one
// frame, computes the 2 R2 + 3 conv1 rows it needs into an LDS tile (same bias + ReLU + fp16 rounding as the unfused
// layer, so conv2's result is bit-identical), and runs conv2 on that tile with its fragments read by ds_read_b128.
// Neighbouring bands recompute 3 conv1 rows each ((2 R2 + 3) / (2 R2) of the conv1 work).
// Measured and dropped (1024 frames of 120x160; this form: 128-131 us):
//   * two wave teams and two tiles (conv1 of the next item beside conv2 of the current one): 8 / 10 / 12 of the 16 waves on
//     conv1 -> 209 / 180 / 160 us - conv1 scales with the waves it gets;
//   * two conv1 tiles requested together per wave (36 dwords in flight): 141 us;
//   * ONE unaligned 8-byte load per k-step instead of three aligned dwords + v_alignbyte: 144 us (267 -> 297 us at 240x320) -
//     the misaligned 8-byte loads cost the addresser more than the three aligned ones.
#ifndef TRS_FUSE_ABLATE
#define TRS_FUSE_ABLATE 0
#endif
#ifndef TRS_C2_ABLATE
#define TRS_C2_ABLATE 0
#endif
#ifndef TRS_C2_NT
#define TRS_C2_NT 1      /* conv2 tiles of the fused head per wave item (one weight fragment feeds that many MFMAs); 2 measured: see the kernel */
#endif
#ifndef TRS_C2_DEPTH
#define TRS_C2_DEPTH 4   /* k-steps of fragments in flight */
#endif
#ifndef TRS_BAND_STAMPS
#define TRS_BAND_STAMPS 0   /* diagnostic build, never shipped: workgroup 7's waves 0 and 8 add up the shader clocks of their phases and print them behind a last barrier */
#endif
#if TRS_BAND_STAMPS
#define BAND_STAMP(i) do { const long long t_ = (long long)__builtin_amdgcn_s_memtime(); st_[i] += t_ - t0_; t0_ = t_; } while (0)
#else
#define BAND_STAMP(i) do { } while (0)
#endif

// The fused head with conv1's input staged once per band.  (Rounds 1-2 had a direct form whose conv1 tiles fetched their windows
// straight from the frame: 18 scattered dword loads and ~100 VALU ops per lane and 32-pixel tile for 6 MFMAs, each frame byte fetched and
// unpacked ~6 times — conv1's phase was 70 of 131 us, bound by the texture addresser; removed in round 4, a frame shape whose band does not
// fit runs the two layers unfused.)  Here the workgroup loads the band's frame rows ONCE (contiguous in the frame: one coalesced 16-byte load per
// thread, requested one item ahead so that its latency hides behind conv1 of the current item), unpacks them once into a fp16
// image in LDS, and conv1 reads its k-steps (8 consecutive values, 4-byte aligned) from there with two ds_read2_b32.
// Same fp16 values as the separate layers; conv2's k dimension runs in column-parity order (see the tile layout below).
template <bool SPLIT>
__global__ __launch_bounds__(1024) void trs_conv12_band_kernel(const Fuse12Params q)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    u4v* lw1 = reinterpret_cast<u4v*>(psmem);                              // [12][32]
    u4v* lw2 = reinterpret_cast<u4v*>(psmem + q.off_w2);                   // [80][32]
    float4* lb1 = reinterpret_cast<float4*>(psmem + q.off_b);              // [8]
    float4* lb2 = lb1 + 8;                                                 // [8]
    // conv1 tile in LDS: [r1 rows][2 planes: even / odd conv1 columns][plane_px][24] fp16.  conv2 (stride 2) reads, per output
    // pixel x2 and kernel row, the conv1 columns 2 x2 .. 2 x2 + 4: with the columns interleaved the 16 lanes of a ds_read_b128
    // group sit 96 bytes apart — an EVEN number of 16-byte slots, so only 8 of the 16 bank groups are hit (2-way conflict on
    // every fragment read, and no padding changes the parity).  Split by column parity, consecutive x2 are 48 bytes = 3 slots
    // apart (odd: all 16 bank groups), and a window is two runs: even columns (3 pixels = 9 slots) then odd (2 pixels = 6
    // slots) — conv2's granules are packed in that order for this kernel (w2 = the handle's parity-ordered copy).
    unsigned char* tile1 = psmem + q.off_tile;
    const int plane_px = SPLIT ? q.w2p + 2 : (q.OW1 + 1) >> 1, plane_bytes = plane_px * 48, tile_pitch = 2 * plane_bytes;   // (a part's conv1 width is 2 w2p + 3)
    unsigned char* band = psmem + q.off_band;                              // [2 r1 + 3][IW * 3] fp16 (+ padding)
    for (int i = tid; i < 12 * 32; i += blockDim.x) lw1[i] = q.w1[i];
    for (int i = tid; i < 80 * 32; i += blockDim.x) lw2[i] = q.w2[i];
    for (int i = tid; i < 8; i += blockDim.x) { lb1[i] = *reinterpret_cast<const float4*>(q.b1 + 4 * i); lb2[i] = *reinterpret_cast<const float4*>(q.c2.bias + 4 * i); }
    for (int i = tid; i < q.tile_bytes / 16; i += blockDim.x) reinterpret_cast<u4v*>(tile1)[i] = (u4v)(0u);   // never multiply an uninitialised bit pattern by a zero weight
    for (int i = tid; i < q.band_bytes / 16; i += blockDim.x) reinterpret_cast<u4v*>(band)[i] = (u4v)(0u);

    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(q.frames), 0, q.frames_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout2 = __builtin_amdgcn_make_buffer_rsrc(static_cast<unsigned char*>(q.c2.out), 0, q.c2.M * 64, 0x00020000);   // conv2's activation: 32 couts
    const float inv_ow2 = 1.0f / (float)q.OW2;
    constexpr bool kC2NtIsOne = TRS_C2_NT == 1;
    const int row_in = q.IW * 3;                                            // bytes per frame row
    const int bpitch = SPLIT ? q.cpr * 16 : row_in;                         // values per row of the band image
    auto divmod = [](int v, int d, float inv, int& qt, int& rm) {
        qt = (int)(((float)v + 0.5f) * inv); rm = v - qt * d;
        if (rm < 0) { --qt; rm += d; } else if (rm >= d) { ++qt; rm -= d; }
    };
    // The workgroup's item `it` = (frame n, band of R2 conv2 rows from y2_0[, part of w2 conv2 columns from x2_0]); w1 = the part's conv1 columns.
    // Two orders (q.roll, chosen by the host):
    //   flat     item blockIdx.x + it * gridDim.x of all (frame, band, part) triples - neighbouring bands go to different workgroups, every band
    //            computes all 2 r2 + 3 conv1 rows under it (3 of them a second time);
    //   rolling  (round 3) the workgroup takes whole (frame, part) streams and walks their bands top to bottom: the conv1 tile is a ring of
    //            NR = 2 R2 + 3 rows (conv1 row y lives in slot y mod NR), the last 3 rows of the previous band are still in it, so a band after
    //            the first computes only its 2 r2 NEW rows (`skip` = 3) from a band image that starts 6 frame rows lower: a fifth less conv1
    //            arithmetic, unpacking and LDS traffic, and 30 instead of 37 conv1 tiles per band at 120x160 (two rounds of the 16 waves, not
    //            three).  Same values into the same MFMAs: bit-identical to the flat order.
    const int NR = 2 * q.R2 + 3;
    auto geometry = [&](int it, int& n, int& y2_0, int& r2, int& r1, int& x2_0, int& w2, int& w1, int& skip) {
        int b, part = 0;
        if (q.roll) {
            const int sidx = it / q.bands;
            b = it - sidx * q.bands;
            const int stream = (int)blockIdx.x + sidx * (int)gridDim.x;
            if constexpr (SPLIT) { n = stream / q.wsplit; part = stream - n * q.wsplit; } else n = stream;
            skip = b > 0 ? 3 : 0;
        } else {
            const int wt = (int)blockIdx.x + it * (int)gridDim.x;
            if constexpr (SPLIT) {
                const int per = q.bands * q.wsplit;
                n = wt / per;
                const int rem = wt - n * per;
                b = rem / q.wsplit; part = rem - b * q.wsplit;
            } else {
                n = wt / q.bands;
                b = wt - n * q.bands;
            }
            skip = 0;
        }
        y2_0 = b * q.R2;
        if constexpr (SPLIT) { x2_0 = min(part * q.w2p, q.OW2 - q.w2p); w2 = q.w2p; w1 = 2 * w2 + 3; }   // every part w2p columns wide: the last one starts where it ends at the frame's edge and
                                                                                                       // recomputes the column(s) it shares with its neighbour (the same values to the same bytes)
        else { x2_0 = 0; w2 = q.OW2; w1 = q.OW1; }
        r2 = min(q.R2, q.OH2 - y2_0); r1 = 2 * (r2 - 1) + 5;
    };
    // the band of item wt: frame rows 4 y2_0 .. + 2 r1 + 2 — whole rows are contiguous in the frame; a part takes 16 cpr bytes of each
    // row from column 4 x2_0 on (what it reads past its own 2 w1 + 3 pixels is never used)
    // A loader thread moves HALF chunks (8 frame bytes -> 16 bytes of the image): consecutive lanes then write consecutive 16-byte
    // slots (whole chunks per lane put the two ds_write_b128 of a lane 32 bytes apart: a 2-way bank conflict on every write)
    auto request = [&](int it, uint2 (&raw)[2 * kBandPf]) {
        int n, y2_0, r2, r1, x2_0, w2, w1, skip;
        geometry(it, n, y2_0, r2, r1, x2_0, w2, w1, skip);
        const int row0 = 4 * y2_0 + 2 * skip, rows = 2 * (r1 - skip) + 3;   // the frame rows under the conv1 rows this item computes
        int tl = tid - 512;                                                  // this loader thread; opaque to the optimiser: the per-chunk indices below are
        asm volatile("" : "+v"(tl));                                         // a few shifts per band, not eight registers held (and spilled) through both phases
        if constexpr (SPLIT) {
            const int start = ((n * q.IH + row0) * q.IW + 4 * x2_0) * 3, nchunk = rows * q.cpr;
#pragma unroll
            for (int j = 0; j < 2 * kBandPf; ++j) {
                const int hc = tl + j * 512, c = hc >> 1, row = (int)__umulhi((unsigned)max(c, 0), q.magic_cpr), kk = c - row * q.cpr;
                raw[j] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rin, c < nchunk ? start + row * row_in + 16 * kk + 8 * (hc & 1) : q.frames_bytes, 0, 0));   // past the end: zeros
            }
        } else {
            const int start = (n * q.IH + row0) * row_in, nchunk = (rows * row_in) >> 4;
#pragma unroll
            for (int j = 0; j < 2 * kBandPf; ++j) {
                const int hc = tl + j * 512;
                raw[j] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rin, (hc >> 1) < nchunk ? start + 8 * hc : q.frames_bytes, 0, 0));   // past the end: zeros
            }
        }
    };
    auto unpack = [&](const uint2 (&raw)[2 * kBandPf]) {                     // 8 uint8 -> 8 fp16 (exact), 16 bytes of the band image
#pragma unroll
        for (int j = 0; j < 2 * kBandPf; ++j) {
            const int hc = (tid - 512) + j * 512;
            if (hc * 16 + 16 > q.band_bytes) continue;
            // two pixels as x / 256 in binary16 (exact: 0, 2^-8 .. 255 x 2^-8) in TWO instructions: binary16's 4.0 (0x4400) has an ulp of 2^-8, so
            // 0x4400 | x IS 4 + x / 256; a byte permute drops the two bytes into the mantissas of (4.0, 4.0) and one packed subtract takes the 4.0 away
            // (until round 4: v_cvt_f32_ubyte x 2, v_cvt_pkrtz, v_pk_mul_f16 — the loader waves share their SIMDs with the conv2 waves, and every
            // vector instruction there is time the MFMAs do not get, profiles/r04_mfma_issue.txt)
            auto pair = [](unsigned w, int k) -> unsigned {
                typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
                const unsigned sel = k == 0 ? 0x05010500u : 0x05030502u;     // result bytes, low to high: w.byte[k], 0x44, w.byte[k + 1], 0x44 (sources 0..3 = w, 4..7 = the magic)
                const unsigned m = __builtin_amdgcn_perm(0x44004400u, w, sel);   // = the halves 0x4400 | w.byte[k], 0x4400 | w.byte[k + 1]
                const h16x2 four = {(_Float16)4.0f, (_Float16)4.0f};
                return __builtin_bit_cast(unsigned, __builtin_bit_cast(h16x2, m) - four);
            };
            *reinterpret_cast<u4v*>(band + (size_t)hc * 16) = u4v{pair(raw[j].x, 0), pair(raw[j].x, 2), pair(raw[j].y, 0), pair(raw[j].y, 2)};
        }
    };

    // Waves 8..15 are the loaders: they have no conv2 tiles (and so no stores in their memory queue to wait behind), request a
    // band a whole item ahead and unpack it while waves 0..7 run conv2.
    const int n_streams = q.N * (SPLIT ? q.wsplit : 1), n_flat = n_streams * q.bands;
    const int mine = q.roll ? n_streams : n_flat;                           // what the workgroups share out: streams of bands, or single items
    const int total = ((int)blockIdx.x < mine ? (mine - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0) * (q.roll ? q.bands : 1);   // this workgroup's items
    const bool loader = wave >= 8;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);                // tile indices in scalar registers
    const unsigned magic1 = (unsigned)((0x100000000ull + (unsigned)q.OW1 - 1u) / (unsigned)q.OW1);   // floor(p / OW1) = umulhi(p, magic1) for p < 65536
    int wt = 0;                                                             // this workgroup's item counter
    uint2 raw[2 * kBandPf];
    if (loader && wt < total) request(wt, raw);
    __syncthreads();                                                        // weights staged, tile and band zeroed
    if (loader && wt < total) {
        unpack(raw);
        if (wt + 1 < total) request(wt + 1, raw);                           // the second item's band is on its way
    }
    __syncthreads();
    // conv1's weights are the same for every tile of every band: this lane's five granules stay in registers for the whole kernel (they were 6 of the
    // 11 LDS reads of a conv1 tile; re-reading them per band — two dependent LDS round trips in front of every band's first tile — was measured in
    // round 4: ~0.5 k of a band's 4 k clocks of phase 1).  So does the bias: it is the first MFMA's C operand (16 registers: couts 8 qd + 4 h + j in
    // register 4 qd + j, zeros for the padding couts 24..31), and the band image holds the pixels as x / 256 (exact), so the sums need no 2^-8 and
    // no bias FMA.
    u4v wv[5];
#pragma unroll
    for (int s6 = 0; s6 < 5; ++s6) wv[s6] = lw1[(2 * s6 + h) * 32 + r];
#pragma unroll
    for (int s6 = 0; s6 < 5; ++s6) asm volatile("" : "+v"(wv[s6]));         // keep them in registers: do not re-read them per tile
    f32x16 bias16;
#pragma unroll
    for (int qd = 0; qd < 3; ++qd) {
        const float4 bb = lb1[2 * qd + h];
        bias16[4 * qd] = bb.x; bias16[4 * qd + 1] = bb.y; bias16[4 * qd + 2] = bb.z; bias16[4 * qd + 3] = bb.w;
    }
#pragma unroll
    for (int i = 12; i < 16; ++i) bias16[i] = 0.0f;
    asm volatile("" : "+v"(bias16));
    // the rolling bands of whole-width frames share one conv1 geometry (2 R2 new rows of OW1 pixels: at most two tiles per wave): this lane's
    // window address in the band image, its column's offset in a ring row, and (pixel index | row << 16) for the tiles wave and wave + 16
    // ... and so do their conv2 tiles (one per wave, kC2Nt = 1): the tile pixel's column address in a ring row, and (row << 24 | byte offset of its 32 output
    // bytes relative to the band's first output pixel); a lane past a full band's last pixel takes that pixel (never stored)
    const int w2c = SPLIT ? q.w2p : q.OW2, w1c = SPLIT ? 2 * q.w2p + 3 : q.OW1;      // conv2 / conv1 columns of an item (the same for every item)
    const bool c2_fast = kC2NtIsOne && (q.R2 * w2c + 31) / 32 <= 8 && q.R2 * q.OW2 * 64 < (1 << 24);
    unsigned c2s_abase = 0, c2s_rel = 0;
    if (c2_fast) {
        const int mm = min(wave_u * 32 + r, q.R2 * w2c - 1);
        const int yl2 = (int)(((float)mm + 0.5f) * (SPLIT ? 1.0f / (float)w2c : inv_ow2));
        int yq = yl2, x2 = mm - yl2 * w2c;
        if (x2 < 0) { --yq; x2 += w2c; } else if (x2 >= w2c) { ++yq; x2 -= w2c; }
        c2s_abase = (unsigned)q.off_tile + (unsigned)__mul24(x2, 48);
        c2s_rel = ((unsigned)yq << 24) | (unsigned)((__mul24(yq, q.OW2) + x2) * 64 + 32 * h);
    }
    struct C1Slot { unsigned ra, pk; };                                     // pk = pixel index (10 bits) | row (4 bits) | column offset in a ring row (the rest)
    C1Slot c1s[2];
    const bool c1_fast = q.roll && (2 * q.R2 * w1c + 31) / 32 <= 2 * nwaves && 2 * q.R2 < 16 && 2 * nwaves * 32 <= 1024;
    if (c1_fast) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int pp = (wave_u + i * nwaves) * 32 + r;
            const int yl = (int)__umulhi((unsigned)pp, SPLIT ? q.magic_full : magic1), x = pp - yl * w1c;
            c1s[i].ra = (unsigned)q.off_band + 16u * h + (unsigned)(__mul24(2 * yl, bpitch) + __mul24(x, 6)) * 2u;   // (past the band's last pixel: still inside the image
                                                                                                                  // buffer, which is sized for a frame's first band; never stored)
            c1s[i].pk = (unsigned)pp | ((unsigned)yl << 10) | ((unsigned)(((x & 1) ? plane_bytes : 0) + __mul24(x >> 1, 48)) << 14);
        }
    }
#if TRS_BAND_STAMPS
    long long st_[5] = {0, 0, 0, 0, 0}, t0_ = (long long)__builtin_amdgcn_s_memtime();
#endif
    while (wt < total) {
        const int nxt = wt + 1;                                             // uniform per workgroup
        int n, y2_0, r2, r1, x2_0, w2, w1, skip;
        geometry(wt, n, y2_0, r2, r1, x2_0, w2, w1, skip);
        const unsigned magic = SPLIT ? q.magic_full : magic1;
        const int s0 = q.roll ? (2 * y2_0) % NR : 0;                        // ring slot of the band's first conv1 row
        // ---- phase 1: the band's conv1 rows that are not in the tile yet (all of them, or all but the first 3), from the fp16 image ----
        const int rows1 = r1 - skip, npx1 = rows1 * w1, ntile1 = (npx1 + 31) >> 5;
#if TRS_FUSE_ABLATE != 1
        // one conv1 tile: five fragments from the band image (kernel rows 0..4 of this lane's window, half h), five MFMAs (the bias is the first one's C
        // operand), ReLU + fp16, three 8-byte writes into the ring (couts 8 qd + 4 h .. + 3, qd = 0..2: 24 channels)
        // (8-byte writes: the two column planes share bank groups, a 2-way conflict.  Swapping halves between the two lanes of a pixel (v_permlane32_swap_b32)
        // to write whole 16-byte granules was measured: head 100.7 -> 103.5 us on one box — the exchange and its selects cost more than the conflict.
        // Requesting the next tile's fragments right behind this tile's MFMAs was measured too: the oldest wave of a SIMD finishes 5 % earlier, the phase —
        // which ends with the youngest — not at all: head 76.0 us against 75.9.)
        auto conv1_tile = [&](unsigned rd, bool mine, unsigned dst_off) {
            u4v xv[5];                                                      // every fragment of the tile first: one LDS round trip, then the MFMAs back to back
#pragma unroll
            for (int s6 = 0; s6 < 5; ++s6) {
                const unsigned* src = reinterpret_cast<const unsigned*>(psmem + (rd + (unsigned)(s6 * bpitch * 2)));
                xv[s6] = u4v{src[0], src[1], src[2], src[3]};
            }
            __builtin_amdgcn_sched_barrier(0);                              // (left alone, hipcc interleaves the reads with the MFMAs two deep to save registers)
            f32x16 acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, wv[0]), __builtin_bit_cast(h16x8, xv[0]), bias16, 0, 0, 0);
#pragma unroll
            for (int s6 = 1; s6 < 5; ++s6)                                  // (the sixth k-step of the padded weight layout is all zeros: skipped, + 0 changes nothing)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h16x8, wv[s6]), __builtin_bit_cast(h16x8, xv[s6]), acc, 0, 0, 0);
            if (mine) {
                uint2* dst = reinterpret_cast<uint2*>(tile1 + dst_off);
                if (q.c1_bounded) {                                         // (wave-uniform: conv1 cannot leave binary16's range with these weights — no saturation step)
#pragma unroll
                    for (int qd = 0; qd < 3; ++qd) dst[2 * qd + h] = relu_pack4_bounded(acc[4 * qd], acc[4 * qd + 1], acc[4 * qd + 2], acc[4 * qd + 3]);
                } else {
#pragma unroll
                    for (int qd = 0; qd < 3; ++qd) dst[2 * qd + h] = relu_pack4(acc[4 * qd], acc[4 * qd + 1], acc[4 * qd + 2], acc[4 * qd + 3]);
                }
            }
        };
        if (c1_fast && skip == 3) {
            // a band after the first of its frame (rolling): 2 R2 new rows, the same geometry for every such band — this lane's windows and columns were
            // worked out once (c1s), only the ring slot of its row moves with the band
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (wave_u + i * nwaves < ntile1) {                         // (wave-uniform)
                    const int ppi = (int)(c1s[i].pk & 1023u), yli = (int)((c1s[i].pk >> 10) & 15u);
                    int slot1 = s0 + 3 + yli;                                // (< 2 NR)
                    slot1 = slot1 >= NR ? slot1 - NR : slot1;
                    conv1_tile(c1s[i].ra, ppi < npx1, (unsigned)__mul24(slot1, tile_pitch) + (c1s[i].pk >> 14));
                }
            }
        } else {
            // the general walk (a frame's first band, bands cut in width, one band per item): a lane walks its pixels p = 32 t1 + r, t1 = wave, wave + 16, ...
            // incrementally: (row yl, column x), the LDS address of its window in the band image and its ring slot in the tile advance by wave-uniform steps
            // with one wrap
            const int step = nwaves * 32;
            const int adv_y = (int)__umulhi((unsigned)step, magic), adv_x = step - adv_y * w1;          // step = adv_y rows + adv_x columns
            const int adv_slot = adv_y % NR;
            int pp = wave_u * 32 + r;
            int yl = (int)__umulhi((unsigned)pp, magic), x = pp - yl * w1;
            const unsigned band_off = (unsigned)q.off_band + 16u * h;
            unsigned ra = band_off + (unsigned)(__mul24(2 * yl, bpitch) + __mul24(x, 6)) * 2u;             // kernel row 0 of this lane's window, half h
            const unsigned ra_last = band_off + (unsigned)(__mul24(2 * (rows1 - 1), bpitch) + (w1 - 1) * 6) * 2u;   // lanes past the band's last pixel compute it again (never stored)
            const unsigned ra_step = (unsigned)(adv_y * 2 * bpitch + adv_x * 6) * 2u, ra_wrap = (unsigned)(2 * bpitch - w1 * 6) * 2u;
            int slot1 = s0 + skip + yl;                                      // (< 2 NR)
            slot1 = slot1 >= NR ? slot1 - NR : slot1;
            for (int t1 = wave_u; t1 < ntile1; t1 += nwaves) {
                conv1_tile(min(ra, ra_last), pp < npx1, (unsigned)(__mul24(slot1, tile_pitch) + ((x & 1) ? plane_bytes : 0) + __mul24(x >> 1, 48)));
                pp += step; x += adv_x; slot1 += adv_slot; ra += ra_step;
                if (x >= w1) { x -= w1; slot1 += 1; ra += ra_wrap; }
                slot1 = slot1 >= NR ? slot1 - NR : slot1;
            }
        }
#endif
        BAND_STAMP(0);                                                      // conv1 tiles
        __syncthreads();                                                    // the tile is complete, the band image is free
        BAND_STAMP(1);                                                      // wait at the barrier
        if (loader) {
            if (nxt < total) {
                unpack(raw);                                                // the next item's band (requested an item ago)
                if (nxt + 1 < total) request(nxt + 1, raw);
            }
        } else {
            // ---- phase 2: conv2 rows from the tile (waves 0..7: at most a handful of tiles per band) ----
            const int npx2 = r2 * w2, ntile2 = (npx2 + 31) >> 5;
            const int m0 = (n * q.OH2 + y2_0) * q.OW2 + x2_0;               // first output pixel of the band (a whole band is consecutive in memory)
            const float inv_w2 = SPLIT ? 1.0f / (float)w2 : inv_ow2;
#if TRS_FUSE_ABLATE != 2
            // Phase stamps of round 4 (-DTRS_BAND_STAMPS=1, profiles/r04_pilot_head_stamps.txt; clocks per band of 7 tiles at 120x160):
            //   * The K loop is bound by LDS bandwidth: every MFMA takes 2 KB out of LDS (its weight and its pixel fragment), 560 KB per band =
            //     4.4 k clocks at 128 B/clk; the waves of a SIMD finish in age order, the phase ends ~4.4 k clocks after it began.
            //   * Until round 4 the epilogue went through a wave-private LDS stage (four broadcast bias reads, then the transpose: six dependent LDS
            //     round trips of ~200 clocks each while the other waves saturate the LDS): 1.4 k clocks per tile.  Now the accumulators start at the
            //     bias and the epilogue is ReLU + fp16 + v_permlane32_swap_b32 + two 16-byte stores per lane, no LDS: ~0.6 k.  Head 95.9 -> 88.5 us.
            //   * TRS_C2_NT = 2 (a wave takes a PAIR of tiles, one weight fragment feeds two MFMAs: 480 KB per band; fragments kC2Depth k-steps ahead
            //     by hand): the pairs run on four waves, one per SIMD, and each needs 3.7 k clocks for its 80 MFMAs + 1.0 k for two epilogues — 95.7 us
            //     on the same box.  (Round 2 measured the same split with compiler-scheduled reads: 107 -> 130 us; conv2's 40 weight fragments in
            //     registers on eight waves of 256 registers 100 -> 117 us, the same with K split over two waves 100 -> 125 us, r02_pilot_head_reg.txt.)
            //   * s_setprio 3 while the loader waves unpack (measured, removed: they finish in 1.0 k instead of 3.0 k clocks, but the conv2 waves
            //     they displace are the critical path): 90.0 us.  Deeper fragment rings (6, 8 k-steps): no change.
            //   * The odd k-steps' weight fragments straight from global memory (buffer loads, three in flight = six k-steps of lead; the LDS then delivers
            //     1.5 KB per MFMA and the L1 the rest): K loop 2.5 k -> 3.5 k clocks per band, head 76.3 -> 81 us (240x320: 162 -> 191) — the frames the
            //     loader waves stream through the same 32 KB L1 evict the weights, and an L2 hit is longer than the lead 128 registers leave room for.
            constexpr int kC2Nt = TRS_C2_NT, kC2Depth = TRS_C2_DEPTH;
            // window slot sl = 2 ks + h of a kernel row (ks = k-step within the row): 0..8 = the even run, 9..14 = the odd run, 15 = padding (zero
            // weights: the odd run's next 16 bytes).  Per lane that is three bases (+ 32 ks as the instruction's immediate offset):
            const unsigned off_lo = 16 * h;                                              // ks 0..3: slots 0..7
            const unsigned off_mid = h ? (unsigned)plane_bytes : 128u;                   // ks 4: slot 8 (even run) / 9 (odd run, first)
            const unsigned off_hi = (unsigned)plane_bytes - 144u + 16 * h;               // ks 5..7: slots 10..15 = odd run + (2 ks + h - 9) * 16
            const unsigned wbase = (unsigned)q.off_w2 + (unsigned)(h * 32 + r) * 16u;    // lw2[(kh * 16 + 2 ks + h) * 32 + r]
            for (int tp = wave_u; kC2Nt * tp < ntile2; tp += 8) {
                unsigned abase[kC2Nt]; int trow[kC2Nt], moff[kC2Nt];
#pragma unroll
                for (int j = 0; j < kC2Nt; ++j) {
                    const int px = (kC2Nt * tp + j) * 32 + r;
                    if (c2_fast) {                                           // (uniform) whole-width band, one tile per wave: this lane's (row, column) were worked out once
                        abase[j] = c2s_abase;
                        trow[j] = s0 + 2 * (int)(c2s_rel >> 24);
                        moff[j] = px < npx2 ? m0 * 64 + (int)(c2s_rel & 0xFFFFFFu) : -1;
                    } else {
                        const int mm = min(px, npx2 - 1);                    // (lanes past the band's last pixel compute it again: never stored)
                        int yl2, x2;
                        divmod(mm, w2, inv_w2, yl2, x2);
                        abase[j] = (unsigned)q.off_tile + (unsigned)__mul24(x2, 48);   // even plane, pixel x2
                        trow[j] = s0 + 2 * yl2;                              // ring slot of conv1 row 2 yl2 + kh: trow + kh (mod NR)
                        moff[j] = px < npx2 ? ((m0 + __mul24(yl2, q.OW2) + x2) * 32 + 16 * h) * 2 : -1;   // this lane's 32 bytes of the pixel in conv2's activation
                    }
                }
                f32x16 acc2[kC2Nt][1];
                acc_from_bias(acc2, lb2, 0, h);                             // the accumulators start at conv2's bias (read once per item, under the first fragments' latency)
                u4v fw[kC2Depth], fx[kC2Depth][kC2Nt];
                unsigned arow[kC2Nt], cur[kC2Nt];
                auto fetch = [&](int k, int d) {                             // k-step k = kernel row k / 8, window slots 2 (k % 8) + h (compile-time k after unrolling)
                    const int kh = k >> 3, ks = k & 7;
#pragma unroll
                    for (int j = 0; j < kC2Nt; ++j) {
                        if (ks == 0) {
                            int tr = trow[j] + kh;
                            tr = tr >= NR ? tr - NR : tr;
                            arow[j] = abase[j] + (unsigned)__mul24(tr, tile_pitch);
                            cur[j] = arow[j] + off_lo;
                        } else if (ks == 4) cur[j] = arow[j] + off_mid;
                        else if (ks == 5) cur[j] = arow[j] + off_hi;
                    }
                    const unsigned imm = ks == 4 ? 0u : 32u * ks;
                    fw[d] = *reinterpret_cast<const u4v*>(psmem + (wbase + (unsigned)(kh * 16 + 2 * ks) * 512u));
#pragma unroll
                    for (int j = 0; j < kC2Nt; ++j) fx[d][j] = *reinterpret_cast<const u4v*>(psmem + (cur[j] + imm));
                };
#pragma unroll
                for (int d = 0; d < kC2Depth; ++d) fetch(d, d);
#pragma unroll
                for (int k = 0; k < 40; ++k) {
                    const int d = k % kC2Depth;
                    const h16x8 w = __builtin_bit_cast(h16x8, fw[d]);
#pragma unroll
                    for (int j = 0; j < kC2Nt; ++j) {
#if TRS_C2_ABLATE == 2
                        asm volatile("" :: "v"(w), "v"(fx[d][j]));
#else
                        acc2[j][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, __builtin_bit_cast(h16x8, fx[d][j]), acc2[j][0], 0, 0, 0);
#endif
                    }
                    if (k + kC2Depth < 40 && TRS_C2_ABLATE != 1) fetch(k + kC2Depth, d);
                    __builtin_amdgcn_sched_barrier(0);
                }
                BAND_STAMP(2);                                               // conv2: set-up and K loop (loaders: unpack + request)
#if TRS_C2_ABLATE == 3
                asm volatile("" :: "v"(acc2[0][0]));
                continue;
#endif
                // Epilogue without LDS: ReLU + fp16, the two lanes of a pixel swap half of their channel quads (v_permlane32_swap_b32) and each stores
                // 32 contiguous bytes (couts 16 h .. + 15).  (Until round 4 the tile went through a wave-private LDS stage — four broadcast bias reads and
                // the transpose, six dependent LDS round trips at ~200 clocks each while the other waves saturate the LDS: 1.4 k of a band's 6.5 k clocks
                // of phase 2 per tile, profiles/r04_pilot_head_stamps.txt.)
#pragma unroll
                for (int j = 0; j < kC2Nt; ++j) {
                    u4v g0, g1;
                    block_groups(acc2[j][0], g0, g1);
                    if (moff[j] >= 0) {
                        __builtin_amdgcn_raw_buffer_store_b128(g0, rout2, moff[j], 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128(g1, rout2, moff[j] + 16, 0, 0);
                    }
                }
            }
#endif
        }
        BAND_STAMP(3);                                                      // conv2: epilogue and stores (loaders: all of phase 2)
        __syncthreads();                                                    // the tile is free, the next band image is complete
        BAND_STAMP(4);                                                      // wait at the barrier
        wt = nxt;
    }
#if TRS_BAND_STAMPS
    __syncthreads();
    if (blockIdx.x == 7 && lane == 0 && (wave == 0 || wave == 3 || wave == 8))
        printf("band head, workgroup 7, wave %d, %d items [clocks]: conv1 tiles %lld | barrier %lld | conv2 K loop %lld | conv2 stores (loaders: phase 2) %lld | barrier %lld\n",
               wave, total, st_[0], st_[1], st_[2], st_[3], st_[4]);
#endif
}
