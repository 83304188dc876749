// trsim_scene.hpp — the scene of a handle: what it renders besides its track's geometry.  Host-only arithmetic that a host compiler builds without HIP
// (tests/scene_driver.cpp runs it on the CPU): which features are set (Scene) and which step-kernel variant that selects, to which colours the host
// applies the static frame filter, and the byte images the kernels read — the flat palette, the lens planes and palette, the table of the
// dynamic-brightness filter and the colour half of the block behind the raster image.  Every builder returns host bytes; allocating and copying is
// trsim_scene.hip's.  The plain structs the kernels read those bytes through (HillBlock, LensBlock, FParams) live here as well: trsim_device.hpp includes
// this header.  Functions the kernels call too carry TRS_HD (trsim_tables.hpp).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_filter.hpp"
#include "trsim_plan.hpp"
#include "trsim_tables.hpp"

namespace trsim {

// ---- what the kernels read (parameter blocks and the blocks behind the raster image) ----

// What the kernels need on a track with elevation.  It lives in device memory BEHIND the raster LDS image's bytes (RParams::blob + hill_block_offset): the kernel
// arguments of the flat-track kernels are exactly what they were before tracks had elevation — arguments sit in scalar registers for the whole kernel, and even one
// more pointer shifted the flat single-step launch by 2-4 % (profiles/r05_hills.txt).  Only the HILLS instantiations ever form this address.
// Two halves: the geometry (hill_geometry: written when a track is committed) and the colours (hill_colours: written with every palette).
struct HillBlock {
    const float* vpitch;                // [np] the view pitch of a frame whose nearest raw track point is idx: (float)pitch + dpitch[idx], one binary32 addition (host)
    float* cam_pitch;                   // [kRing][n_envs] ring of the frames' view pitches beside PParams::cam (launch mode: the next launch's first frame)
    int off_sky;                        // raster LDS image: uint32 sky[H] (the sky colour of every row; filtered by the host when a frame filter is set)
    unsigned far_rgb;                   // (likewise)
    float inv_f, hh, cam_h_f, z_far_f, inv_zfar_f, fog_f, inv_cell_f;
    // the static frame filter (trs_set_frame_filter without dynamic brightness) on a track with elevation: the ground colours of a row are blended per env and
    // frame, so the filter of ONE colour (img_preprocessing.py:37-74,92-99: the host's filter_colour) runs on each of them in hill_row_build
    int filt, f_color, f_nfilters;
    float f_contrast, f_offset;
    unsigned f_lo[4], f_hi[4];          // packed h | s << 8 | v << 16
    int f_dst[4];
    const int* hsv_tab;                 // [512] OpenCV's sdiv | hdiv fixed-point reciprocals (global)
    // scene lighting (trs_set_lighting; the LIGHT instantiations only, flat tracks included): the caller's float[n_envs][8] {gR gG gB 0 bR bG bB 0}.  With lighting
    // set, the host keeps the palette, the sky colours and the far colour RAW and fills the static frame filter above: the kernels light, then filter
    const float* light;
};
TRS_HD inline size_t hill_block_offset(int blob_bytes) { return ((size_t)blob_bytes + 63) & ~(size_t)63; }

// What the LENS instantiations need (include/trsim_spec.h, "lens camera"): like HillBlock it lives in device memory behind the raster image, so the
// flat kernels' arguments stay as they are.  The per-pixel table is stored for the RIGHT half of the frame only (u = W/2 + k, k in [0, W/2)): F, depth
// and the palette row are even in u - W/2 and L is odd, so pixel W-1-u reads entry k with L negated.  Planes of [H][W/2], so that the 4 pixels of a
// thread's column group are one 16-B load per plane (8 B for the rows).
struct LensBlock {
    const float* F;                     // [H][W/2] forward distance, cell units
    const float* L;                     // [H][W/2] lateral distance, cell units (right half: + = right)
    const float* D;                     // [H][W/2] z-depth (z_far for sky and far pixels)
    const uint16_t* M;                  // [H][W/2] lens palette row: 0..255 ground G(q), 256..511 sky S(q), 512 FAR
    const uint32_t* pal;                // [513][4] the lens palette (static frame filter applied), staged into LDS by the kernels
    float oc;                           // (float)(offset_x / cell): the lateral mount, cell units
    int wh;                             // W/2
};
TRS_HD inline size_t lens_block_offset(int blob_bytes) { return hill_block_offset(blob_bytes) + ((sizeof(HillBlock) + 63) & ~(size_t)63); }

struct FParams {                        // ImgPreprocessing with dynamic brightness, evaluated inside the step kernels (their DYN instantiations)
    double baseline;
    float contrast, offset;
    int color, n_filters;
    int lo[4], hi[4], dst_ch[4];
    int w0, w1;                         // brightness window: image rows [w0, w1) = img[40:119] (img_preprocessing.py:88)
    int lds_off;                        // LDS: uint32 penv[4][H][4] | int esum[2][4][3] | int dbar | (128 B) | dyn tables (kDynTabWords)
    const unsigned* tabs;               // global, kDynTabWords (dyn_table): int hsv[512] (OpenCV's sdiv | hdiv fixed-point reciprocals) | rngb[768] (byte masks of the
                                        // in-range tests per component value, range_byte_entry) | sel — staged into LDS once per launch (round 4: the
                                        // resident worker's raster waves then issue NO loads in their steady state)
};
constexpr int kDynCntAt = 512 + 768 + 4;

// entry i = c * 256 + x of the colour masks' table (mask_pixel, trsim_device.hpp): byte ch = 0xFF when value x of component c (h, s, v) lies inside the range
// of the filter whose mask goes to channel ch (a later filter on the same channel replaces an earlier one); *sel_out = the channels that carry a mask
TRS_HD inline unsigned range_byte_entry(const unsigned (&lo)[4], const unsigned (&hi)[4], const int (&dst_ch)[4], int n_filters, int i, unsigned* sel_out)
{
    const int c = i >> 8, x = i & 255;
    int fsel[3] = {-1, -1, -1};
    for (int f = 0; f < n_filters; ++f) { const int dc = dst_ch[f]; if (dc >= 0 && dc <= 2) fsel[dc] = f; }
    unsigned word = 0, sel = 0;
    for (int ch = 0; ch < 3; ++ch) {
        if (fsel[ch] < 0) continue;
        const int l = (int)((lo[fsel[ch]] >> (8 * c)) & 255u), u = (int)((hi[fsel[ch]] >> (8 * c)) & 255u);
        sel |= 0xFFu << (8 * ch);
        if (x >= l && x <= u) word |= 0xFFu << (8 * ch);
    }
    if (sel_out) *sel_out = sel;
    return word;
}

// ---- a filter's HSV bounds as every kernel takes them ----

// one HSV bound of a colour filter (trs_pre_config::hsv_lo / hsv_hi): h | s << 8 | v << 16
inline unsigned pack_hsv(const uint8_t (&b)[3]) { return (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16); }
struct FilterBounds { unsigned lo[4], hi[4]; int dst[4]; };
inline FilterBounds filter_bounds(const trs_pre_config& c)
{
    FilterBounds b;
    for (int k = 0; k < 4; ++k) {
        b.lo[k] = pack_hsv(c.hsv_lo[k]);
        b.hi[k] = pack_hsv(c.hsv_hi[k]);
        b.dst[k] = c.dst_channel[k];
    }
    return b;
}

// ---- the scene's state ----

struct Scene {
    bool hilly = false;                 // the loaded track has elevation (include/trsim_spec.h): the HILLS instantiations of the kernels run
    bool lens_on = false;               // the lens camera (trs_set_camera; "lens camera"): the LENS instantiations run
    bool light_on = false;              // scene lighting (trs_set_lighting; "scene lighting"): the LIGHT instantiations run
    bool has_filter = false;            // trs_set_frame_filter: `filter` is set
    trs_pre_config filter{};
    trs_camera camera{};                // what trs_set_camera set (all zero: the pinhole)
    HillBlock hill{};                   // the geometry half of the block behind the raster image, as the track's commit wrote it (hill_geometry)

    // dynamic brightness: the DYN kernels filter a per-env palette with each frame's own delta
    bool dynamic_filter() const { return has_filter && filter.dynamic_brightness != 0; }
    // a filter without it is the same for every frame: the host applies it to the constant colours, the kernels to the colours they blend (HillBlock::filt)
    bool static_filter() const { return has_filter && filter.dynamic_brightness == 0; }
    // lighting comes first (the LIGHT kernels light a colour, then filter it): the host leaves raw what those kernels will light
    bool lit_first() const { return light_on; }
    void drop_filter() { has_filter = false; }
    // the instantiation of the step kernel and of the resident worker that this state selects (Variant, trsim_plan.hpp); depth: the handle writes depth frames
    Variant variant(bool depth) const { return variant_bits(depth, dynamic_filter(), hilly, lens_on, light_on); }
};

// The static frame filter on n colours the host holds — the only place the host filters a palette.  lightable: the colours go through the LIGHT kernels when
// lighting is set (the flat palette, the sky, the far colour), so they stay raw then.  The lens palette is not lightable: a lens excludes lighting
// (variant_clash), no LENS kernel lights, and its palette is filtered whatever light_on says.
inline void host_filter(const Scene& s, bool lightable, uint32_t* colours, size_t n)
{
    if (!s.static_filter() || (lightable && s.lit_first())) return;
    for (size_t i = 0; i < n; ++i) colours[i] = filter_colour(s.filter, colours[i]);
}

// The in-kernel dynamic filter keeps the class bits of a thread's brightness rows in 4 registers: 16 rows of 2 bits x 4 pixels each.  A thread owns every
// rows_per_pass-th row of the window, which is at its longest for frames of dyn_window_hi's limit or more rows.
inline bool dyn_filter_width_ok(int W)
{
    const int rpp = raster_rows_per_pass(W / 4), window = dyn_window_hi(INT_MAX) - dyn_window_lo(INT_MAX);
    return rpp >= 1 && (window + rpp - 1) / rpp <= 16;
}

// ---- the byte images ----

// The palette of the raster LDS image as uploaded, and how many leading rows of it have four equal colours (RParams::uni_rows: sky, beyond the far plane).
// No row counts as uniform on a track with elevation (which rows are sky depends on the env and the frame) or under a lens (on the pixel).
struct FlatPalette { std::vector<uint32_t> pal; int uni_rows = 0; };
inline FlatPalette flat_palette(const Scene& s, const TrackTables& T, int H)
{
    FlatPalette p;
    p.pal = T.palette;
    host_filter(s, true, p.pal.data(), p.pal.size());
    auto uniform = [&](int r) { const uint32_t* c = &p.pal[4 * (size_t)r]; return c[0] == c[1] && c[0] == c[2] && c[0] == c[3]; };
    if (!(s.hilly || s.lens_on))
        while (p.uni_rows < H && uniform(p.uni_rows)) ++p.uni_rows;
    return p;
}

inline std::vector<uint32_t> lens_palette(const Scene& s, const LensTables& T)
{
    std::vector<uint32_t> lp(T.palette);
    host_filter(s, false, lp.data(), lp.size());
    return lp;
}

// The device image of a lens camera's tables: planes F | L | D | M of [H][W/2] (the RIGHT half of the frame, see LensBlock; M = the low 16 bits of channel 3's bit
// pattern), each starting on a multiple of 256 bytes, F at 0, then the lens palette (kLensPalBytes) at off_pal.
struct LensImage { std::vector<unsigned char> bytes; size_t off_L = 0, off_D = 0, off_M = 0, off_pal = 0; };
inline LensImage lens_image(const Scene& s, const LensTables& T)
{
    const int H = T.H, W = T.W, wh = W / 2;
    const size_t plane = ((size_t)H * wh * 4 + 255) / 256 * 256, mplane = ((size_t)H * wh * 2 + 255) / 256 * 256;
    LensImage im;
    im.off_L = plane; im.off_D = 2 * plane; im.off_M = 3 * plane; im.off_pal = 3 * plane + mplane;
    im.bytes.assign(im.off_pal + (size_t)kLensPalBytes, 0);
    unsigned char* const h = im.bytes.data();
    for (int v = 0; v < H; ++v)
        for (int k = 0; k < wh; ++k) {
            const float* px = &T.pix[((size_t)v * W + wh + k) * 4];
            const size_t i = (size_t)v * wh + k;
            uint32_t row;
            std::memcpy(&row, &px[3], 4);
            const uint16_t m = (uint16_t)row;
            std::memcpy(h + i * 4, &px[0], 4);
            std::memcpy(h + im.off_L + i * 4, &px[1], 4);
            std::memcpy(h + im.off_D + i * 4, &px[2], 4);
            std::memcpy(h + im.off_M + i * 2, &m, 2);
        }
    const std::vector<uint32_t> lp = lens_palette(s, T);
    std::memcpy(h + im.off_pal, lp.data(), lp.size() * 4);
    return im;
}

// FParams::tabs of a dynamic-brightness filter, kDynTabWords: OpenCV's reciprocals [512] | the in-range byte masks of THIS filter [768] | sel (+ 3 spare) |
// the class counts of a 4-pixel pack of 2-bit classes [256]: n0 | n1 << 8 | n2 << 16 | n3 << 24
inline std::vector<unsigned> dyn_table(const trs_pre_config& c)
{
    std::vector<unsigned> t(kDynTabWords, 0u);
    hsv_reciprocals(reinterpret_cast<int*>(t.data()));      // (the same 512 words the device's hsv table holds)
    const FilterBounds b = filter_bounds(c);
    unsigned sel = 0;
    for (int i = 0; i < 768; ++i) t[512 + i] = range_byte_entry(b.lo, b.hi, b.dst, c.n_filters, i, &sel);
    t[512 + 768] = sel;
    for (int i = 0; i < 256; ++i) {
        unsigned cnt = 0;
        for (int k = 0; k < 4; ++k) cnt += 1u << (8 * ((i >> (2 * k)) & 3));
        t[kDynCntAt + i] = cnt;
    }
    return t;
}

// the dynamic-brightness filter that is set, as the DYN instantiations take it (all zero without one); H: the frame's rows, tabs: the device copy of
// dyn_table, lds_off: the filter's region in the kernel's LDS layout
inline FParams dyn_fparams(const Scene& s, int H, const unsigned* tabs, int lds_off)
{
    FParams f;
    std::memset(&f, 0, sizeof f);
    if (!s.dynamic_filter()) return f;
    const trs_pre_config& c = s.filter;
    f.baseline = c.brightness_baseline; f.contrast = c.contrast_ratio; f.offset = c.contrast_offset;
    f.color = c.color_filter_enabled; f.n_filters = c.n_filters;
    const FilterBounds b = filter_bounds(c);
    for (int k = 0; k < 4; ++k) { f.lo[k] = (int)b.lo[k]; f.hi[k] = (int)b.hi[k]; f.dst_ch[k] = b.dst[k]; }
    f.w0 = dyn_window_lo(H); f.w1 = dyn_window_hi(H);       // img[40:119] (img_preprocessing.py:88)
    f.tabs = tabs;
    f.lds_off = lds_off;
    return f;
}

// The geometry half of a track's HillBlock.  vpitch and cam_pitch are device addresses: the caller sets them.
inline HillBlock hill_geometry(const TrackTables& T, int off_sky)
{
    HillBlock hb{};
    hb.off_sky = off_sky;
    hb.inv_f = T.inv_f; hb.hh = T.hh; hb.cam_h_f = T.cam_h_f; hb.z_far_f = T.z_far_f; hb.inv_zfar_f = T.inv_zfar_f; hb.fog_f = T.fog_f; hb.inv_cell_f = T.inv_cellf;
    return hb;
}

// The colour half, into a copy of the geometry half; returns the sky colours of the raster image (HillBlock::off_sky; a track with elevation only).
// On a track with elevation the kernels blend a row's ground colours per env and frame and run the static filter on each (hill_filter_colour): filt and
// the f_* fields; a flat track's LIGHT kernels read the filter from this block as well.  The sky colours and the far colour are constants: lightable, like
// the flat palette.  hsv_tab (needed when filt is set) and light are device addresses: the caller sets them.
inline std::vector<uint32_t> hill_colours(const Scene& s, const TrackTables& T, HillBlock& hb)
{
    std::vector<uint32_t> sky(T.sky);
    host_filter(s, true, sky.data(), sky.size());
    hb.far_rgb = T.far_rgb;
    host_filter(s, true, &hb.far_rgb, 1);
    hb.filt = s.static_filter() ? 1 : 0;
    if (hb.filt) {
        const trs_pre_config& c = s.filter;
        hb.f_color = c.color_filter_enabled; hb.f_nfilters = c.n_filters; hb.f_contrast = c.contrast_ratio; hb.f_offset = c.contrast_offset;
        const FilterBounds b = filter_bounds(c);
        std::memcpy(hb.f_lo, b.lo, sizeof b.lo); std::memcpy(hb.f_hi, b.hi, sizeof b.hi); std::memcpy(hb.f_dst, b.dst, sizeof b.dst);
    }
    return sky;
}

}  // namespace trsim
