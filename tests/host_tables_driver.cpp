// Test driver (CPU): runs the PRODUCT's host-side table builder (triton-racer-sim_amd/csrc/trsim_tables.cpp) on a config and a
// track handed over in files, and writes the tables out; tests/test_host_tables.py builds it with AddressSanitizer +
// UBSan and compares the tables with the oracle's bit for bit.  With <envs_per_wg> it also lays out the track's two LDS images
// (trsim_plan.hpp: track_layout, pack_track_images), prints the layout (or the refusal) and writes the images and the members they hold.
//   host_tables_driver <config.bin> <points.bin> <out_prefix> [<envs_per_wg>]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_plan.hpp"
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
    if (argc != 4 && argc != 5) return 2;
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
    const int rc = trsim::build_tables(cfg, xyz.data(), (int)(xyz.size() / 3), t, err);
    if (rc) { std::fprintf(stderr, "build_tables: %d %s\n", rc, err.c_str()); return rc == 0 ? 1 : 10; }
    const std::string p = argv[3];
    dump(p + ".map", t.map); dump(p + ".rowtab", t.rowtab); dump(p + ".palette", t.palette); dump(p + ".tangent", t.tangent);
    dump(p + ".rowdepth", t.rowdepth);
    std::printf("%d %d %d %d\n", t.n_points, t.info.map_w, t.info.map_h, t.info.map_words);
    if (argc == 5) {
        trsim::TrackLayout L;
        const int rl = trsim::track_layout(t, cfg.img_h, cfg.render != 0, std::atoi(argv[4]), L, err);
        if (rl) { std::printf("refused %d %s\n", rl, err.c_str()); return 0; }
        std::printf("layout p.off_py=%d p.off_pz=%d p.off_tan=%d p.tan_in_lds=%d p.off_gstart=%d p.off_gpts=%d p.blob_bytes=%d p.off_scratch=%d p.pts_bytes=%d p.lds_p=%d "
                    "r.map_pitch_b=%d r.off_rowtab=%d r.off_pal=%d r.off_depth=%d r.off_sky=%d r.blob_bytes=%d r.lds_r=%d lds_off_phys=%d lds_step=%d\n",
                    L.p.off_py, L.p.off_pz, L.p.off_tan, L.p.tan_in_lds, L.p.off_gstart, L.p.off_gpts, L.p.blob_bytes, L.p.off_scratch, L.p.pts_bytes, L.p.lds_p,
                    L.r.map_pitch_b, L.r.off_rowtab, L.r.off_pal, L.r.off_depth, L.r.off_sky, L.r.blob_bytes, L.r.lds_r, L.lds_off_phys, L.lds_step);
        std::vector<unsigned char> phys, raster;
        trsim::pack_track_images(t, cfg.img_h, L, phys, raster);
        dump(p + ".phys", phys); dump(p + ".raster", raster);
        dump(p + ".px", t.px); dump(p + ".py", t.py); dump(p + ".pz", t.pz); dump(p + ".grid_start", t.grid_start); dump(p + ".grid_pts", t.grid_pts); dump(p + ".sky", t.sky);
        std::printf("hills %d\n", t.hills ? 1 : 0);
    }
    return 0;
}
