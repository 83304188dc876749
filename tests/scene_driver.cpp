// Test driver (CPU): the host-only owner of a handle's scene (triton-racer-sim_amd/csrc/trsim_scene.hpp) on the PRODUCT's tables
// (trsim_tables.cpp) for tests/test_scene_cpu.py, which builds it with AddressSanitizer + UBSan.
//   scene_driver scene <config.bin> <points.bin> <pre.bin | -> <light 0|1> <lens 0|1> <fish_eye_x> <fish_eye_y> <out_prefix>
//       the scene of a handle with that track, frame filter (the bytes of a trs_pre_config; -: none), lighting and lens camera.  Files: .raw (the tables'
//       palette), .pal (flat_palette), .sky (hill_colours); with a lens .lens (the full-frame table), .lensraw (its palette), .lenspal (lens_palette),
//       .lensimg (lens_image); with a dynamic filter .dyn (dyn_table).  Lines: variant, uni_rows, hill (the block's colour half), lensimg (offsets),
//       fparams (bounds and window)
//   scene_driver bounds <pre.bin>     one config's bounds as filter_bounds packs them, as the hill block holds them (the config as a static filter) and as
//                                     FParams holds them (as a dynamic one)
//   scene_driver width                dyn_filter_width_ok of every width that is a multiple of 4 up to 1024
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_scene.hpp"

static std::vector<unsigned char> slurp(const char* path)
{
    std::vector<unsigned char> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(3); }
    unsigned char buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path.c_str()); std::exit(3); }
    std::fclose(f);
}

static trs_pre_config pre_of(const char* path)
{
    const std::vector<unsigned char> b = slurp(path);
    trs_pre_config c;
    const char* why = nullptr;
    if (b.size() != sizeof c) { std::fprintf(stderr, "bad trs_pre_config size\n"); std::exit(3); }
    std::memcpy(&c, b.data(), sizeof c);
    if (trsim::check_pre(&c, &why)) { std::fprintf(stderr, "%s\n", why); std::exit(2); }
    return c;
}

static void print4(const char* tag, const unsigned (&lo)[4], const unsigned (&hi)[4], const int (&dst)[4])
{
    std::printf("%s", tag);
    for (int k = 0; k < 4; ++k) std::printf(" %u %u %d", lo[k], hi[k], dst[k]);
    std::printf("\n");
}

static void print_hill(const trsim::HillBlock& hb)
{
    std::printf("hill %u %d %d %d %.9g %.9g\n", hb.far_rgb, hb.filt, hb.f_color, hb.f_nfilters, hb.f_contrast, hb.f_offset);
    print4("hill_bounds", hb.f_lo, hb.f_hi, hb.f_dst);
}

static void print_fparams(const trsim::FParams& f)
{
    unsigned lo[4], hi[4];
    for (int k = 0; k < 4; ++k) { lo[k] = (unsigned)f.lo[k]; hi[k] = (unsigned)f.hi[k]; }
    std::printf("fparams %d %d %d %d %.9g %.9g %.17g %d\n", f.w0, f.w1, f.color, f.n_filters, f.contrast, f.offset, f.baseline, f.lds_off);
    print4("fparams_bounds", lo, hi, f.dst_ch);
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "width")) {
        for (int W = 4; W <= 1024; W += 4) std::printf("%d %d\n", W, trsim::dyn_filter_width_ok(W) ? 1 : 0);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "bounds")) {
        trsim::Scene s;
        s.filter = pre_of(argv[2]); s.has_filter = true;
        const trsim::FilterBounds b = trsim::filter_bounds(s.filter);
        print4("bounds", b.lo, b.hi, b.dst);
        trsim::TrackTables none;
        trsim::HillBlock hb{};
        s.filter.dynamic_brightness = 0;
        (void)trsim::hill_colours(s, none, hb);
        print_hill(hb);
        s.filter.dynamic_brightness = 1;
        print_fparams(trsim::dyn_fparams(s, 120, nullptr, 0));
        return 0;
    }
    if (argc != 10 || std::strcmp(argv[1], "scene")) { std::fprintf(stderr, "usage: scene_driver scene ... | bounds <pre.bin> | width\n"); return 1; }
    const std::vector<unsigned char> cb = slurp(argv[2]), pb = slurp(argv[3]);
    trs_config cfg;
    if (cb.size() != sizeof cfg || pb.size() % (3 * sizeof(double))) { std::fprintf(stderr, "bad input sizes\n"); return 3; }
    std::memcpy(&cfg, cb.data(), sizeof cfg);
    std::vector<double> xyz(pb.size() / sizeof(double));
    std::memcpy(xyz.data(), pb.data(), pb.size());
    trsim::TrackTables T;
    std::string err;
    int rc = trsim::build_tables(cfg, xyz.data(), (int)(xyz.size() / 3), T, err);
    if (rc) { std::fprintf(stderr, "build_tables: %d %s\n", rc, err.c_str()); return 10; }

    trsim::Scene s;
    s.hilly = T.hills;
    if (std::strcmp(argv[4], "-")) { s.filter = pre_of(argv[4]); s.has_filter = true; }
    s.light_on = std::atoi(argv[5]) != 0;
    s.lens_on = std::atoi(argv[6]) != 0;
    const std::string p = argv[9];
    std::printf("variant %u\n", s.variant(cfg.depth != 0));

    const trsim::FlatPalette fp = trsim::flat_palette(s, T, cfg.img_h);
    dump(p + ".raw", T.palette); dump(p + ".pal", fp.pal);
    std::printf("uni_rows %d\n", fp.uni_rows);

    trsim::HillBlock hb = trsim::hill_geometry(T, 0);
    dump(p + ".sky", trsim::hill_colours(s, T, hb));
    print_hill(hb);

    if (s.lens_on) {
        trsim::LensTables L;
        rc = trsim::build_lens_tables(cfg, T.info.cell, std::strtod(argv[7], nullptr), std::strtod(argv[8], nullptr), L, err);
        if (rc) { std::fprintf(stderr, "build_lens_tables: %d %s\n", rc, err.c_str()); return 11; }
        const trsim::LensImage im = trsim::lens_image(s, L);
        dump(p + ".lens", L.pix); dump(p + ".lensraw", L.palette); dump(p + ".lenspal", trsim::lens_palette(s, L)); dump(p + ".lensimg", im.bytes);
        std::printf("lensimg %zu %zu %zu %zu %zu\n", im.off_L, im.off_D, im.off_M, im.off_pal, im.bytes.size());
    }
    if (s.dynamic_filter()) dump(p + ".dyn", trsim::dyn_table(s.filter));
    print_fparams(trsim::dyn_fparams(s, cfg.img_h, nullptr, 0));
    return 0;
}
