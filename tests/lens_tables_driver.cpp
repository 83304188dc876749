// Test driver (CPU): runs the PRODUCT's host-side table builders (triton-racer-sim_amd/csrc/trsim_tables.cpp) for the lens camera on a config, a track
// and two fish-eye strengths handed over in files / arguments, and writes the lens table, the lens palette and the flat row tables out;
// tests/test_lens_tables_cpu.py builds it with AddressSanitizer + UBSan and compares them with a numpy restatement of include/trsim_spec.h bit for bit.
//   lens_tables_driver <config.bin> <points.bin> <fish_eye_x> <fish_eye_y> <out_prefix>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_tables.hpp"

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::perror(path.c_str()); std::exit(3); }
    std::fwrite(v.data(), sizeof(T), v.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 6) return 2;
    trs_config cfg;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&cfg, sizeof cfg, 1, f) != 1) return 3;
    std::fclose(f);
    f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<double> xyz(bytes / sizeof(double));
    if (std::fread(xyz.data(), sizeof(double), xyz.size(), f) != xyz.size()) return 3;
    std::fclose(f);
    trsim::TrackTables t;
    std::string err;
    int rc = trsim::build_tables(cfg, xyz.data(), (int)(xyz.size() / 3), t, err);
    if (rc) { std::fprintf(stderr, "build_tables: %d %s\n", rc, err.c_str()); return 10; }
    trsim::LensTables L;
    rc = trsim::build_lens_tables(cfg, t.info.cell, std::strtod(argv[3], nullptr), std::strtod(argv[4], nullptr), L, err);
    if (rc) { std::fprintf(stderr, "build_lens_tables: %d %s\n", rc, err.c_str()); return 11; }
    const std::string p = argv[5];
    dump(p + ".lens", L.pix); dump(p + ".lenspal", L.palette); dump(p + ".rowtab", t.rowtab); dump(p + ".palette", t.palette);
    std::printf("%.17g %d %d\n", t.info.cell, L.H, L.W);
    return 0;
}
