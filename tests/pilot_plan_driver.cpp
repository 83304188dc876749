// Test driver (CPU): the pilot's plan and weight packing (triton-racer-sim_amd/csrc/trsim_pilot_plan.hpp, the header alone) printed for
// tests/test_pilot_plan_cpu.py, which builds it with AddressSanitizer + UBSan, and for tests/test_pilot.py, which asks it which kernel a case reaches.
//   pilot_plan_driver plan <H | lo:hi> <W> <n_cap> <cus> <arrays> [field=value ...]
//       the plan of trs_pilot_load with the default tuning and the given trs_pilot_tuning fields on top: per H one line per layer, a head line and
//       a chain line, or one refuse line
//   pilot_plan_driver call <H> <W> <n_cap> <cus> <arrays> <n | lo:hi> [field=value ...]
//       per batch n one line: dense1's K slices and frame grouping, the head's roll flag and grid, and the grid of every layer launched by itself
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

#include "../triton-racer-sim_amd/csrc/trsim_pilot_plan.hpp"

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

// what serves conv(i + 1) in a forward pass, as trsim_pilot.hip's forward dispatches: the fused head, the chain, else the layer's own kernel
static const char* pilot_served_by(const PilotPlan& P, int i)
{
    static const char* const names[] = {"u8", "span<1>", "span<2>", "lt<1>", "lt<2>", "frame", "frame5"};   // in PilotKernel's order
    if (i < 2 && pilot_head_runs(P)) return P.head.wsplit > 1 ? "band<split>" : "band<whole>";
    if (P.chain.first >= 0 && i >= P.chain.first && i < 7) return "chain";
    return names[pilot_kernel_of(P.L[i])];
}

static void print_plan(const PilotPlan& P)
{
    if (P.err) { std::printf("refuse H=%d W=%d n_cap=%d code=%d text=%s\n", P.H, P.W, P.n_cap, P.err, P.err_text); return; }
    for (int i = 0; i < P.n_layers; ++i) {
        const PilotLayer& l = P.L[i];
        std::printf("layer H=%d W=%d n_cap=%d i=%d KH=%d KW=%d S=%d CIN=%d COUT=%d COUT_PAD=%d IH=%d IW=%d OH=%d OW=%d G=%d G_pad=%d run_pad=%d "
                    "res_nb=%d res_ysplit=%d res_block=%d res_lds=%d res_wg_per_cu=%d res_span=%d span_nl=%d frame=%d frame_f=%d frame_bands=%d frame_ohb=%d frame_lds=%d "
                    "frame5=%d frame5_bands=%d frame5_ohb=%d frame5_lds=%d served_by=%s\n",
                    P.H, P.W, P.n_cap, i, l.KH, l.KW, l.S, l.CIN, l.COUT, l.COUT_PAD, l.IH, l.IW, l.OH, l.OW, l.G, l.G_pad, i < 7 ? l.run_pad : 0,
                    l.res_nb, l.res_ysplit, l.res_block, l.res_lds, l.res_wg_per_cu, (int)l.res_span, l.span_nl, (int)l.frame, l.frame_f, l.frame_bands, l.frame_ohb, l.frame_lds,
                    (int)l.frame5, l.frame5_bands, l.frame5_ohb, l.frame5_lds, i < 7 ? pilot_served_by(P, i) : "dense");
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
    const bool plan = argc >= 7 && !std::strcmp(argv[1], "plan"), call = argc >= 8 && !std::strcmp(argv[1], "call");
    if (plan || call) {
        int h_lo, h_hi, n_lo = 0, n_hi = 0;
        range(argv[2], &h_lo, &h_hi);
        const int W = std::atoi(argv[3]), n_cap = std::atoi(argv[4]), cus = std::atoi(argv[5]), arrays = std::atoi(argv[6]);
        if (call) range(argv[7], &n_lo, &n_hi);
        trs_pilot_tuning T = pilot_default_tuning();
        if (!tuning(&T, argc, argv, call ? 8 : 7)) return 2;
        for (int H = h_lo; H <= h_hi; ++H) {
            const PilotPlan P = pilot_plan(H, W, n_cap, cus, arrays, T);
            if (plan || P.err) { print_plan(P); continue; }
            for (int n = n_lo; n <= n_hi; ++n) {
                const DenseCall d = dense_call(P.L[7], n, cus, T);
                const HeadCall hc = head_call(P, n);
                std::printf("call H=%d W=%d n_cap=%d n=%d G=%d nf=%d gps=%d KS=%d groups=%d dense_grid=%d dense_lds=%d head_runs=%d roll=%d head_grid=%d chain_grid=%d",
                            H, W, n_cap, n, P.L[7].G, d.nf, d.gps, d.KS, d.groups, d.grid, d.lds, (int)pilot_head_runs(P), hc.roll, hc.grid, P.chain.first >= 0 ? chain_grid(P.chain, n) : 0);
                for (int i = 0; i < 7; ++i) {
                    const PilotLayer& l = P.L[i];
                    const PilotKernel k = pilot_kernel_of(l);
                    std::printf(" grid%d=%d", i, k == kKernFrame5 ? frame5_grid(l, n, cus) : k == kKernFrame ? frame_grid(l, n, cus) : single_grid_x(l, n, cus));
                }
                std::printf("\n");
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
