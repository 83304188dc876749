// Test driver (CPU): the pilot's plan, weight packing and passes (triton-racer-sim_amd/csrc/trsim_pilot_plan.hpp and trsim_pilot_pass.hpp, the headers alone) printed for
// tests/test_pilot_plan_cpu.py, which builds it with AddressSanitizer + UBSan, and for tests/test_pilot.py, which asks it which kernel a case reaches.
//   pilot_plan_driver plan <H | lo:hi> <W> <n_cap> <cus> <arrays> [field=value ...]
//       the plan of trs_pilot_load with the default tuning and the given trs_pilot_tuning fields on top: per H one line per layer, a head line and
//       a chain line, or one refuse line
//   pilot_plan_driver call <H | lo:hi> <W> <n_cap> <cus> <arrays> <n | lo:hi> [show=brief] [field=value ...]
//       the forward pass of a batch of n (pilot_pass, trsim_pilot_pass.hpp): one call line — dense1's K slices and frame grouping, the head's roll flag and grid, the
//       grid of every layer launched by itself, the two validity flags after the pass — then one launch record per launch and behind each its parameter
//       block(s) with every member but the pointers; a batch the pass refuses is one refuse line.  show=brief: the call (or refuse) lines only
//   pilot_plan_driver materialise <H | lo:hi> <W> <n_cap> <cus> <arrays> <n> <lo> <hi> <act0_valid> <chain_mid_valid> [show=brief] [field=value ...]
//       what pilot_materialise schedules for layers lo..hi after a pass of n frames that left the two flags as given (each of the four may be a range a:b:
//       every lo <= hi of it): one line with the layers launched, their sources and the flags afterwards, then the records of `call`
//   pilot_plan_driver pack <layer> <ih> <iw> <kernel.bin> <bias.bin> <out prefix>
//       layer 0..7 of the network over an ih x iw input, packed from the float32 Keras arrays in the two files: <prefix>.w (uint16 granules),
//       <prefix>.goff (int32), <prefix>.bias (float32); conv2 also <prefix>.parity (the granules in the band kernel's order) and a line with the
//       16 source granules of a kernel row; conv1 also a line with c1_bounded
//   pilot_plan_driver blob <H> <W> <arrays> <dir> <out prefix>
//       the tail kernels' blob of small fp32 weights (pack_tail_blob) from the 28 or 42 float32 Keras arrays in <dir>/a<k>.bin, every one on the heap at exactly
//       its file's size, so that a read past the end of one stops the sanitizer build: <prefix>.blob (float32) and a line with the widths and the XO_* offsets
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_pilot_pass.hpp"

using namespace trsim;

static void range(const char* s, int* lo, int* hi)
{
    const char* colon = std::strchr(s, ':');
    *lo = std::atoi(s); *hi = colon ? std::atoi(colon + 1) : *lo;
}

static bool tuning(trs_pilot_tuning* t, int argc, char** argv, int from)
{
    struct Field { const char* name; int32_t* at; };
    const Field fields[] = {{"no_fuse", &t->no_fuse}, {"fuse_band_r2", &t->fuse_band_r2}, {"fuse_wsplit_max", &t->fuse_wsplit_max}, {"fuse_roll", &t->fuse_roll},
                            {"span_layers_mask", &t->span_layers_mask}, {"frame5", &t->frame5}, {"frame_layers_mask", &t->frame_layers_mask},
                            {"chain_layers", &t->chain_layers}, {"dense", &t->dense}, {"ksplit", &t->ksplit}};
    for (int a = from; a < argc; ++a) {
        const char* eq = std::strchr(argv[a], '=');
        bool found = false;
        for (const Field& f : fields)
            if (eq && std::string(argv[a], (size_t)(eq - argv[a])) == f.name) { *f.at = (int32_t)std::strtol(eq + 1, nullptr, 0); found = true; }
        if (!found) { std::fprintf(stderr, "unknown tuning field: %s\n", argv[a]); return false; }
    }
    return true;
}

template <typename T>
static bool write_file(const std::string& path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

static std::vector<float> read_floats(const char* path)
{
    std::vector<float> v;
    if (FILE* f = std::fopen(path, "rb")) {
        std::fseek(f, 0, SEEK_END);
        v.resize((size_t)std::ftell(f) / sizeof(float));
        std::fseek(f, 0, SEEK_SET);
        if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) v.clear();
        std::fclose(f);
    }
    return v;
}

// what serves conv(i + 1) in a forward pass: the kind of the launch of pilot_pass that computes it (no kind depends on the batch)
static const char* served_by(const PilotPass& pass, int i)
{
    for (int k = 0; k < pass.count; ++k)
        if (pass.at[k].first <= i && i <= pass.at[k].last) return pilot_launch_name(pass.at[k].kind);
    return "nothing";
}

static unsigned bits_of(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

static void print_conv(const char* tag, int k, const ConvParams& p)
{
    std::printf("%s k=%d in_bytes=%d N=%d IH=%d IW=%d CIN=%d OH=%d OW=%d COUT=%d COUT_PAD=%d S=%d G=%d G_pad=%d M=%d in_px_bytes=%d nt_out=%d KH=%d KW=%d run_pad=%d cg=%d span_nl=%d oscale_bits=%u\n",
                tag, k, p.in_bytes, p.N, p.IH, p.IW, p.CIN, p.OH, p.OW, p.COUT, p.COUT_PAD, p.S, p.G, p.G_pad, p.M, p.in_px_bytes, p.nt_out, p.KH, p.KW, p.run_pad, p.cg, p.span_nl, bits_of(p.oscale));
}

// a schedule: one launch record per entry and, behind each, the parameter block trsim_pilot.hip would launch it with (every member but the pointers)
static void print_schedule(const PilotPlan& P, const PilotPass& pass, int n)
{
    for (int k = 0; k < pass.count; ++k) {
        const PilotLaunch& a = pass.at[k];
        const PilotLayer& l = P.L[a.first];
        std::printf("launch k=%d kind=%s first=%d last=%d src=%d dst=%d in_bytes=%zu grid_x=%d grid_y=%d block=%d lds=%d lds_max=%d\n",
                    k, pilot_launch_name(a.kind), a.first, a.last, a.src, a.dst, a.in_bytes, a.grid_x, a.grid_y, a.block, a.lds, a.lds_max);
        switch (a.kind) {
        case kLaunchHeadWhole: case kLaunchHeadSplit: {
            const Fuse12Params q = fuse12_call(fuse12_params(P, 1), P, n, pass.head);
            std::printf("fuse12 k=%d frames_bytes=%d N=%d IH=%d IW=%d OH1=%d OW1=%d OH2=%d OW2=%d R2=%d bands=%d off_w2=%d off_b=%d off_tile=%d tile_bytes=%d off_band=%d band_bytes=%d "
                        "wsplit=%d w2p=%d cpr=%d roll=%d c1_bounded=%d magic_full=%u magic_cpr=%u\n",
                        k, q.frames_bytes, q.N, q.IH, q.IW, q.OH1, q.OW1, q.OH2, q.OW2, q.R2, q.bands, q.off_w2, q.off_b, q.off_tile, q.tile_bytes, q.off_band, q.band_bytes,
                        q.wsplit, q.w2p, q.cpr, q.roll, q.c1_bounded, q.magic_full, q.magic_cpr);
            print_conv("fuse12_c2", k, q.c2);
            break;
        }
        case kLaunchFrame5: {
            const Frame5Params q = frame5_params(l, n);
            std::printf("frame5 k=%d N=%d IH=%d IW=%d OH=%d OW=%d F=%d ev=%d COUT=%d bands=%d ohb=%d ihb=%d magic_ow=%u\n",
                        k, q.N, q.IH, q.IW, q.OH, q.OW, q.F, q.ev, q.COUT, q.bands, q.ohb, q.ihb, q.magic_ow);
            break;
        }
        case kLaunchFrame8: case kLaunchFrame16: {
            const FrameConvParams q = frame_params(l, n);
            std::printf("frame k=%d N=%d IH=%d IW=%d OH=%d OW=%d COUT=%d COUT_PAD=%d KH=%d KW=%d F=%d cg=%d cgs=%d bands=%d ohb=%d ihb=%d magic_uout=%u magic_ow=%u magic_bands=%u instance=%d\n",
                        k, q.N, q.IH, q.IW, q.OH, q.OW, q.COUT, q.COUT_PAD, q.KH, q.KW, q.F, q.cg, q.cgs, q.bands, q.ohb, q.ihb, q.magic_uout, q.magic_ow, q.magic_bands,
                        a.kind == kLaunchFrame8 ? 8 : 16);
            break;
        }
        case kLaunchChain: {
            const ChainParams q = chain_call(chain_params(P), n);
            std::printf("chain_block k=%d N=%d F=%d nl=%d split_first=%d offA=%d offB=%d off_bias=%d", k, q.N, q.F, q.nl, q.split_first, q.offA, q.offB, q.off_bias);
            for (int j = 0; j < q.nl; ++j) {
                const ChainLayer& c = q.L[j];
                std::printf(" IH%d=%d IW%d=%d OH%d=%d OW%d=%d COUT%d=%d cg%d=%d cgs%d=%d nt%d=%d nb%d=%d magic_uout%d=%u magic_ow%d=%u",
                            j, c.IH, j, c.IW, j, c.OH, j, c.OW, j, c.COUT, j, c.cg, j, c.cgs, j, c.nt, j, c.nb, j, c.magic_uout, j, c.magic_ow);
            }
            std::printf("\n");
            break;
        }
        case kLaunchDense1: case kLaunchDense2: {
            const DenseParams q = dense_params(l, pass.dense, n);
            std::printf("dense k=%d n=%d G=%d gps=%d KS=%d groups=%d nf=%d\n", k, q.n, q.G, q.gps, q.KS, q.groups, a.kind == kLaunchDense2 ? 2 : 1);
            break;
        }
        default: print_conv("conv", k, conv_params(l, n));
        }
    }
}

static void print_plan(const PilotPlan& P)
{
    if (P.err) { std::printf("refuse H=%d W=%d n_cap=%d code=%d text=%s\n", P.H, P.W, P.n_cap, P.err, P.err_text); return; }
    const PilotPass pass = pilot_pass(P, 1);
    for (int i = 0; i < P.n_layers; ++i) {
        const PilotLayer& l = P.L[i];
        std::printf("layer H=%d W=%d n_cap=%d i=%d KH=%d KW=%d S=%d CIN=%d COUT=%d COUT_PAD=%d IH=%d IW=%d OH=%d OW=%d G=%d G_pad=%d run_pad=%d "
                    "res_nb=%d res_ysplit=%d res_block=%d res_lds=%d res_wg_per_cu=%d res_span=%d span_nl=%d frame=%d frame_f=%d frame_bands=%d frame_ohb=%d frame_lds=%d "
                    "frame5=%d frame5_bands=%d frame5_ohb=%d frame5_lds=%d served_by=%s\n",
                    P.H, P.W, P.n_cap, i, l.KH, l.KW, l.S, l.CIN, l.COUT, l.COUT_PAD, l.IH, l.IW, l.OH, l.OW, l.G, l.G_pad, i < 7 ? l.run_pad : 0,
                    l.res_nb, l.res_ysplit, l.res_block, l.res_lds, l.res_wg_per_cu, (int)l.res_span, l.span_nl, (int)l.frame, l.frame_f, l.frame_bands, l.frame_ohb, l.frame_lds,
                    (int)l.frame5, l.frame5_bands, l.frame5_ohb, l.frame5_lds, served_by(pass, i));
    }
    const PilotHead& h = P.head;
    if (!h.on) std::printf("head H=%d W=%d n_cap=%d on=0 runs=0\n", P.H, P.W, P.n_cap);
    else std::printf("head H=%d W=%d n_cap=%d on=1 runs=%d R2=%d bands=%d wsplit=%d w2p=%d cpr=%d off_w2=%d off_b=%d off_tile=%d off_band=%d tile_bytes=%d band_bytes=%d lds=%d magic_full=%u magic_cpr=%u\n",
                     P.H, P.W, P.n_cap, (int)pilot_head_runs(P), h.R2, h.bands, h.wsplit, h.w2p, h.cpr, h.off_w2, h.off_b, h.off_tile, h.off_band, h.tile_bytes, h.band_bytes, h.lds, h.magic_full, h.magic_cpr);
    const PilotChain& c = P.chain;
    std::printf("chain H=%d W=%d n_cap=%d first=%d nl=%d F=%d split_first=%d offA=%d offB=%d off_bias=%d lds=%d", P.H, P.W, P.n_cap, c.first, c.nl, c.F, c.split_first, c.offA, c.offB, c.off_bias, c.lds);
    for (int j = 0; j < c.nl; ++j) std::printf(" nt%d=%d nb%d=%d magic_uout%d=%u magic_ow%d=%u", j, c.nt[j], j, c.nb[j], j, c.magic_uout[j], j, c.magic_ow[j]);
    std::printf("\n");
}

int main(int argc, char** argv)
{
    const bool plan = argc >= 7 && !std::strcmp(argv[1], "plan"), call = argc >= 8 && !std::strcmp(argv[1], "call"), mat = argc >= 12 && !std::strcmp(argv[1], "materialise");
    if (plan || call || mat) {
        int h_lo, h_hi, n_lo = 0, n_hi = 0, lo_lo = 0, lo_hi = 0, hi_lo = 0, hi_hi = 0, a0_lo = 0, a0_hi = 0, cm_lo = 0, cm_hi = 0;
        range(argv[2], &h_lo, &h_hi);
        const int W = std::atoi(argv[3]), n_cap = std::atoi(argv[4]), cus = std::atoi(argv[5]), arrays = std::atoi(argv[6]);
        if (call || mat) range(argv[7], &n_lo, &n_hi);
        if (mat) { range(argv[8], &lo_lo, &lo_hi); range(argv[9], &hi_lo, &hi_hi); range(argv[10], &a0_lo, &a0_hi); range(argv[11], &cm_lo, &cm_hi); }
        int from = mat ? 12 : call ? 8 : 7;
        const bool brief = argc > from && !std::strcmp(argv[from], "show=brief");
        from += brief;
        trs_pilot_tuning T = pilot_default_tuning();
        if (!tuning(&T, argc, argv, from)) return 2;
        for (int H = h_lo; H <= h_hi; ++H) {
            const PilotPlan P = pilot_plan(H, W, n_cap, cus, arrays, T);
            if (plan || P.err) { print_plan(P); continue; }
            for (int n = n_lo; n <= n_hi; ++n) {
                if (mat) {
                    for (int lo = lo_lo; lo <= lo_hi; ++lo) for (int hi = std::max(lo, hi_lo); hi <= hi_hi; ++hi) for (int a0 = a0_lo; a0 <= a0_hi; ++a0) for (int cm = cm_lo; cm <= cm_hi; ++cm) {
                        const PilotPass s = pilot_materialise(P, n, lo, hi, a0 != 0, cm != 0);
                        std::printf("materialise H=%d W=%d n_cap=%d n=%d lo=%d hi=%d act0_valid=%d chain_mid_valid=%d code=%d count=%d layers=", H, W, n_cap, n, lo, hi, a0, cm, s.err, s.count);
                        for (int k = 0; k < s.count; ++k) std::printf("%s%d", k ? "," : "", s.at[k].first);
                        std::printf("%s srcs=", s.count ? "" : "-");
                        for (int k = 0; k < s.count; ++k) std::printf("%s%d", k ? "," : "", s.at[k].src);
                        std::printf("%s after_act0_valid=%d after_chain_mid_valid=%d chain_first=%d head_runs=%d%s%s\n", s.count ? "" : "-", (int)s.act0_valid, (int)s.chain_mid_valid, P.chain.first, (int)pilot_head_runs(P),
                                    s.err ? " text=" : "", s.err ? s.err_text : "");
                        if (!brief) print_schedule(P, s, n);
                    }
                    continue;
                }
                const PilotPass s = pilot_pass(P, n);
                if (s.err) { std::printf("refuse H=%d W=%d n_cap=%d n=%d code=%d text=%s\n", H, W, n_cap, n, s.err, s.err_text); continue; }
                const bool head_runs = s.at[0].kind == kLaunchHeadWhole || s.at[0].kind == kLaunchHeadSplit;
                int chain_grid_x = 0;
                for (int k = 0; k < s.count; ++k) if (s.at[k].kind == kLaunchChain) chain_grid_x = s.at[k].grid_x;
                std::printf("call H=%d W=%d n_cap=%d n=%d G=%d nf=%d gps=%d KS=%d groups=%d dense_grid=%d dense_lds=%d head_runs=%d roll=%d head_grid=%d chain_grid=%d",
                            H, W, n_cap, n, P.L[7].G, s.dense.nf, s.dense.gps, s.dense.KS, s.dense.groups, s.dense.grid, s.dense.lds, (int)head_runs, s.head.roll, s.head.grid, chain_grid_x);
                for (int i = 0; i < 7; ++i) std::printf(" grid%d=%d", i, layer_launch(P, i, n).grid_x);   // every layer launched by itself
                std::printf(" count=%d act0_valid=%d chain_mid_valid=%d\n", s.count, (int)s.act0_valid, (int)s.chain_mid_valid);
                if (!brief) print_schedule(P, s, n);
            }
        }
        return 0;
    }
    if (argc >= 8 && !std::strcmp(argv[1], "pack")) {
        const int i = std::atoi(argv[2]);
        if (i < 0 || i > 7) return 3;
        const PilotLayer l = pilot_layer_geometry(i, std::atoi(argv[3]), std::atoi(argv[4]));
        const std::vector<float> K = read_floats(argv[5]), B = read_floats(argv[6]);
        if (l.OH < 1 || l.OW < 1 || K.size() != (size_t)l.KH * l.KW * l.CIN * l.COUT || B.size() != (size_t)l.COUT) return 3;
        const PackedLayer p = pack_layer(l, K.data(), B.data());
        const std::string out = argv[7];
        std::printf("packed G=%d G_pad=%d COUT_PAD=%d run=%d run_pad=%d in_bytes=%zu\n", l.G, l.G_pad, l.COUT_PAD, l.run, l.run_pad,
                    (size_t)l.IH * l.IW * (l.u8in ? 3 : l.CIN * 2));
        if (!write_file(out + ".w", p.w) || !write_file(out + ".goff", p.goff) || !write_file(out + ".bias", p.bias)) return 4;
        if (i == 0) std::printf("c1_bounded %d\n", conv1_bounded(l, K.data(), B.data()));
        if (i == 1) {
            if (!write_file(out + ".parity", conv2_parity_order(l, p.w))) return 4;
            std::printf("parity");
            for (int sl = 0; sl < 16; ++sl) std::printf(" %d", conv2_parity_src(sl));
            std::printf("\n");
        }
        return 0;
    }
    if (argc >= 7 && !std::strcmp(argv[1], "blob")) {
        const int arrays = std::atoi(argv[4]);
        const PilotPlan P = pilot_plan(std::atoi(argv[2]), std::atoi(argv[3]), 1, 256, arrays, pilot_default_tuning());
        if (P.err || (arrays != 22 && arrays != 28 && arrays != 42)) return 3;
        std::vector<std::unique_ptr<float[]>> held;
        std::vector<const float*> arr;
        for (int k = 0; k < arrays; ++k) {
            const std::vector<float> v = read_floats((std::string(argv[5]) + "/a" + std::to_string(k) + ".bin").c_str());
            if (v.empty()) return 3;
            held.emplace_back(new float[v.size()]);                    // exactly the array: no capacity beyond it
            std::copy(v.begin(), v.end(), held.back().get());
            arr.push_back(held.back().get());
        }
        const TailBlob b = pack_tail_blob(P, arr.data());
        std::printf("blob arch=%d F=%d f1=%d f2=%d f3=%d floats=%zu slots=%d", P.arch, P.L[7].CIN, b.f1, b.f2, b.f3, b.data.size(), (int)XO_COUNT);
        for (int k = 0; k < XO_COUNT; ++k) std::printf(" xo%d=%d", k, b.xo[k]);
        std::printf("\n");
        return write_file(std::string(argv[6]) + ".blob", b.data) ? 0 : 4;
    }
    return 2;
}
