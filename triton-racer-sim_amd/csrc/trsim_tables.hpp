// trsim_tables.hpp — host-side (one-time, at trs_load_track) construction of the read-only tables the
// step kernel stages into LDS: per-point tangents / start headings, the packed 2-bit surface-class map,
// the per-image-row camera table and the per-row fogged palette.  Follows include/trsim_spec.h; all of
// it is binary64 arithmetic with IEEE +,-,*,/,sqrt,floor plus libm tan/sin/cos/atan2/fmod evaluated on
// the host, built with -ffp-contract=off.
//
// Track input: the raw [x,y,z] samples the reference's LocationTracker loads
// (TritonRacerSim/components/track_data_process.py:72-73), duplicates kept.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/trsim.h"

namespace trsim {

struct TrackTables {
    int n_points = 0;
    std::vector<double> px, py, pz;        // raw points (SoA, binary64)
    std::vector<float> tangent;            // [n][2] unit (tx, tz)
    std::vector<float> start_yaw;          // [n]
    trs_map_info info{};
    std::vector<uint32_t> map;             // [map_h][map_words], 16 cells per word, cell ix at bits 2*(ix&15)
    std::vector<float> rowtab;             // [H][2]
    std::vector<float> rowdepth;           // [H] z-depth of the ground plane per image row (z_far for sky / far rows)
    std::vector<uint32_t> palette;         // [H][4] 0x00BBGGRR
    float map_x0f = 0, map_z0f = 0, inv_cellf = 0;
    // tracks with elevation (include/trsim_spec.h): the per-point view-pitch offsets and what the kernels need to evaluate a frame's row tables per env
    bool hills = false;
    std::vector<float> dpitch;             // [n]; all zeros on a flat track
    std::vector<uint32_t> sky;             // [H] sky colour of every image row
    uint32_t far_rgb = 0;                  // colour of the rows beyond the far plane
    float inv_f = 0, hh = 0, pitch_f = 0, cam_h_f = 0, z_far_f = 0, inv_zfar_f = 0, fog_f = 0;
    // nearest-point accelerator (trsim_spec.h R3): points bucketed by (x, z) cell, ascending index inside a cell
    int grid_nx = 0, grid_nz = 0;
    double grid_x0 = 0, grid_z0 = 0;
    std::vector<uint16_t> grid_start;      // [grid_nx * grid_nz + 1]
    std::vector<uint16_t> grid_pts;        // [n_points]
};

// The lens camera (include/trsim_spec.h, "lens camera"): per pixel of the full frame F, L, depth and the lens palette row, and the lens palette,
// in binary64 on the host.  The lateral offset is not in the table (the kernels move the camera by it), so the table depends on the config, the
// map's cell size and the two fish-eye strengths only.
constexpr int kLensPalRows = 513;          // 256 ground rows G(q) | 256 sky rows S(q) | FAR
constexpr int kLensSkyRow0 = 256, kLensFarRow = 512;
struct LensTables {
    int H = 0, W = 0;
    std::vector<float> pix;                // [H][W][4]: F, L, depth (binary32), palette row (uint32 bit pattern)
    std::vector<uint32_t> palette;         // [kLensPalRows][4] 0x00BBGGRR, unfiltered
};
int build_lens_tables(const trs_config& cfg, double cell, double kx, double ky, LensTables& out, std::string& err);

// Scene lighting (include/trsim_spec.h, "scene lighting"): one channel value x of a raw rendered colour under gain g and bias b, binary32 with every operation
// rounded (R1: the host and the kernels are built with -ffp-contract=off); NaN goes to 0.  gb = {gR, gG, gB, 0, bR, bG, bB, 0} (the per-env layout of
// trs_set_lighting), colours 0x00BBGGRR.  Host and device share this code: the kernels light palette entries with it, tests/light_driver.cpp checks it.
#if defined(__HIPCC__)
#define TRS_HD __host__ __device__
#else
#define TRS_HD
#endif
TRS_HD inline uint32_t light_channel(uint32_t x, float g, float b)
{
    float t = (float)x * g;
    t = t + b;
    t = t + 0.5f;
    return !(t > 0.0f) ? 0u : (t >= 255.0f ? 255u : (uint32_t)(int)t);
}
TRS_HD inline uint32_t light_colour(uint32_t bgr, const float* gb)
{
    return light_channel(bgr & 255u, gb[0], gb[4]) | (light_channel((bgr >> 8) & 255u, gb[1], gb[5]) << 8) | (light_channel((bgr >> 16) & 255u, gb[2], gb[6]) << 16);
}

// returns TRS_OK or a negative trs_status, message in `err`
int build_tables(const trs_config& cfg, const double* xyz, int n_points, TrackTables& out, std::string& err);

}  // namespace trsim
