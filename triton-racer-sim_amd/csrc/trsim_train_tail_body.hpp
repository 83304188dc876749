// trsim_train_tail_body.hpp — the body of trs_train_tail_kernel, trs_train_tail_drop_kernel and their two SIDE siblings (trsim_train.hip), included once in
// each: no include guard.  The including kernel declares `p` (TailTrainParams), `dp` (TailDropParams), `sd` (TailSideParams), `constexpr bool DROP`,
// `constexpr bool SIDE` and the six LDS arrays s1, s2, s3, e4, e3, e2.  The
// kernels share this text and not a function: inlined from a function template, the plain kernel's code object was no longer the one it is (registers
// allocated otherwise); expanded in place it is, instruction for instruction (scripts/kernel_diff.py).
// DROP (include/trsim_spec.h, "training the pilot's tail, dropout"): a'(l) = keep ? relu(z(l)) s : +0 replaces relu(z(l)) and is stored; delta(l) =
// keep and z(l) > 0 ? (W(l+1) delta(l+1)) s : +0.  Lane k draws the units it owns: the frame's key per site, then one mix per unit (trsim_dropout.hpp).
// SIDE (include/trsim_spec.h, "training the pilot's tail, side branch"): the branch fin -> y1 -> y2 -> y3 runs first (side_forward), the rows W1Y of dense1
// behind the flatten are added to z1 behind the slabs, k ascending, as trs_pilot_tail_ex_kernel adds them, and delta1 goes on through W1Y and the branch
// (side_backward).  The LDS of both is theirs, so the plain kernels declare none of it.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= p.n) return;                                // whole waves
    // z1: the slabs in slice order (what trs_pilot_tail_kernel's padded groups add: x + 0.0f == x), then the ReLU
    const bool two = lane + 64 < 100;
    bool k1a = true, k1b = true, k2 = true, k3 = true;
    if constexpr (DROP) {
        const uint64_t key1 = dropout_frame_key(dp.Dt, 1u, (uint32_t)i), key2 = dropout_frame_key(dp.Dt, 2u, (uint32_t)i), key3 = dropout_frame_key(dp.Dt, 3u, (uint32_t)i);
        k1a = dropout_keep(key1, (uint32_t)lane, dp.T[0]); k1b = dropout_keep(key1, (uint32_t)lane + 64u, dp.T[0]);
        k2 = dropout_keep(key2, (uint32_t)lane, dp.T[1]); k3 = dropout_keep(key3, (uint32_t)lane, dp.T[2]);
    }
    float* ys = nullptr;                                 // SIDE: the wave's y1 | y2 | y3 in LDS
    if constexpr (SIDE) ys = side_forward(sd, i, lane, wv);
    float z1a = 0.0f, z1b = 0.0f;
    for (int sl = 0; sl < p.slices; ++sl) {
        const float* src = p.h1 + (size_t)sl * p.stride + (size_t)i * 100 + lane;
        z1a += src[0];
        z1b += src[two ? 64 : 0];
    }
    if constexpr (SIDE) {
        float wa[kSideRows], wb[kSideRows];
#pragma unroll
        for (int k = 0; k < kSideRows; ++k) { wa[k] = sd.w1y[k * 100 + lane]; wb[k] = sd.w1y[k * 100 + lane + (two ? 64 : 0)]; }
#pragma unroll
        for (int k = 0; k < kSideRows; ++k) { z1a = fmaf(ys[12 + k], wa[k], z1a); z1b = fmaf(ys[12 + k], wb[k], z1b); }
    }
    if constexpr (DROP) {
        const float aa = k1a ? (z1a > 0.f ? z1a : 0.f) * dp.s[0] : 0.f, ab = k1b ? (z1b > 0.f ? z1b : 0.f) * dp.s[0] : 0.f;
        p.z1[(size_t)i * 100 + lane] = z1a; s1[wv][lane] = aa; dp.a1[(size_t)i * 100 + lane] = aa;
        if (two) { p.z1[(size_t)i * 100 + lane + 64] = z1b; s1[wv][lane + 64] = ab; dp.a1[(size_t)i * 100 + lane + 64] = ab; }
    } else {
    p.z1[(size_t)i * 100 + lane] = z1a; s1[wv][lane] = z1a > 0.f ? z1a : 0.f;
    if (two) { p.z1[(size_t)i * 100 + lane + 64] = z1b; s1[wv][lane + 64] = z1b > 0.f ? z1b : 0.f; }
    }
    __builtin_amdgcn_wave_barrier();
    float z2 = 0.0f, z3 = 0.0f;
    if (lane < 50) {                                     // one fmaf chain per output from the bias, k ascending
        float s = p.b2[lane];
        for (int k = 0; k < 100; ++k) s = fmaf(s1[wv][k], p.w2[k * 50 + lane], s);
        z2 = s; p.z2[(size_t)i * 50 + lane] = s;
        if constexpr (DROP) { const float a = k2 ? (s > 0.f ? s : 0.f) * dp.s[1] : 0.f; s2[wv][lane] = a; dp.a2[(size_t)i * 50 + lane] = a; }
        else s2[wv][lane] = s > 0.f ? s : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 25) {
        float s = p.b3[lane];
        for (int k = 0; k < 50; ++k) s = fmaf(s2[wv][k], p.w3[k * 25 + lane], s);
        z3 = s; p.z3[(size_t)i * 25 + lane] = s;
        if constexpr (DROP) { const float a = k3 ? (s > 0.f ? s : 0.f) * dp.s[2] : 0.f; s3[wv][lane] = a; dp.a3[(size_t)i * 25 + lane] = a; }
        else s3[wv][lane] = s > 0.f ? s : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 2) {
        float s = p.b4[lane];
        for (int k = 0; k < 25; ++k) s = fmaf(s3[wv][k], p.w4[k * 2 + lane], s);
        p.out[(size_t)i * 2 + lane] = s;
        const float d = (s - p.y[(size_t)i * 2 + lane]) / (float)p.n;          // delta4
        p.d4[(size_t)i * 2 + lane] = d; e4[wv][lane] = d;
    }
    __builtin_amdgcn_wave_barrier();
    // delta(l) = (W(l+1) delta(l+1)) . [z(l) > 0]: lane k owns row k; one fmaf chain from 0, the output index ascending
    if (lane < 25) {
        float s = 0.0f;
        for (int o = 0; o < 2; ++o) s = fmaf(p.w4[lane * 2 + o], e4[wv][o], s);
        if constexpr (DROP) s = (k3 && z3 > 0.f) ? s * dp.s[2] : 0.0f;
        else s = z3 > 0.f ? s : 0.0f;
        p.d3[(size_t)i * 25 + lane] = s; e3[wv][lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < 50) {
        float s = 0.0f;
        for (int o = 0; o < 25; ++o) s = fmaf(p.w3[lane * 25 + o], e3[wv][o], s);
        if constexpr (DROP) s = (k2 && z2 > 0.f) ? s * dp.s[1] : 0.0f;
        else s = z2 > 0.f ? s : 0.0f;
        p.d2[(size_t)i * 50 + lane] = s; e2[wv][lane] = s;
    }
    __builtin_amdgcn_wave_barrier();
    float da = 0.0f, db = 0.0f;
    {
        const int kb = two ? lane + 64 : lane;
        for (int o = 0; o < 50; ++o) { da = fmaf(p.w2[lane * 50 + o], e2[wv][o], da); db = fmaf(p.w2[kb * 50 + o], e2[wv][o], db); }
        if constexpr (DROP) {
            da = (k1a && z1a > 0.f) ? da * dp.s[0] : 0.0f;
            db = (two && k1b && z1b > 0.f) ? db * dp.s[0] : 0.0f;
        } else {
        da = z1a > 0.f ? da : 0.0f;
        db = (two && z1b > 0.f) ? db : 0.0f;
        }
        p.d1[(size_t)i * 100 + lane] = da;
        if (two) p.d1[(size_t)i * 100 + lane + 64] = db;
    }
    if constexpr (SIDE) side_backward(sd, ys, da, db, two, i, lane, wv);
    wave_max_bits(max(__float_as_uint(da) & 0x7FFFFFFFu, __float_as_uint(db) & 0x7FFFFFFFu), p.max_bits, lane);   // the batch's largest |delta1|
