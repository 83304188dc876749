// trsim_jpeg_decode.hip — the tub image decoder: baseline JPEG files on the device -> uint8[n][H][W][3] frames, byte for byte what include/trsim_spec.h
// ("tub image (JPEG), decoding") defines, which is what Pillow's decoder gives.  Every rule comes from trsim_jpeg_decode.hpp; this file holds the data
// movement of trs_jpeg_decode_kernel up to the sample buffers and the two entry points; the buffers' layout and the way from them to the frame are
// trsim_jpeg_device.hpp's, shared with the camera codec.
// One wave per file, kDecodeWaves independent waves per workgroup, no workgroup barrier.  A file's Huffman decoding is a serial chain: the wave runs it
// as wave-uniform code (every lane computes the same values from the same LDS words), so that the 64 lanes are at hand, without a branch, for what is
// parallel: refilling the window of file bytes, clearing and transforming blocks, upsampling, colour and the stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/trsim.h"
#include "trsim_env.hpp"
#include "trsim_internal.hpp"
#include "trsim_jpeg_device.hpp"
#include "trsim_jpeg_host.hpp"

namespace {
namespace jpeg = trsim::jpeg;
using jpeg::wave_sync;

struct DecodeParams {
    const uint8_t* files; const int64_t* off; const int32_t* len;
    uint8_t* dst; int32_t* status;
    int n, H, W;
    jpeg::DecodeLds lds;
};

extern __shared__ __attribute__((aligned(16))) unsigned char dsmem[];

// The file type of the shared rules on the device: kWindowBytes of the file in the wave's LDS, refilled by all lanes when a byte outside it is asked
// for.  at() must be called by all 64 lanes with the same index.  Global memory is read by aligned dwords that lie wholly inside the file and by bytes
// at its two ends: nothing outside [0, len) is read.
struct WindowFile {
    const uint8_t* g; int len; uint8_t* win; int lo, lane;
    __device__ int size() const { return len; }
    __device__ int at(int i)
    {
        if ((unsigned)i >= (unsigned)len) return 0;
        if ((unsigned)(i - lo) >= (unsigned)jpeg::kWindowBytes) load(i);
        return win[i - lo];
    }
    __device__ void load(int i)
    {
        const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3);
        lo = ((i + mis) & ~3) - mis;                                  // g + lo is dword-aligned; lo may be down to -3
        wave_sync();                                                  // every lane has read what it wanted from the old window
        for (int d = lane; d < jpeg::kWindowBytes / 4; d += 64) {
            const int a = lo + 4 * d;
            uint32_t v = 0;
            if (a >= 0 && a + 4 <= len) {
                v = *reinterpret_cast<const uint32_t*>(g + a);
            } else {
                for (int k = 0; k < 4; ++k)
                    if ((unsigned)(a + k) < (unsigned)len) v |= (uint32_t)g[a + k] << (8 * k);
            }
            reinterpret_cast<uint32_t*>(win)[d] = v;
        }
        wave_sync();
    }
};

__global__ __launch_bounds__(64 * jpeg::kDecodeWaves) void trs_jpeg_decode_kernel(DecodeParams p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned char* base = dsmem + wave * p.lds.wave_bytes;
    jpeg::DecodeTables* T = reinterpret_cast<jpeg::DecodeTables*>(base + p.lds.off_tab);
    int16_t* coef = reinterpret_cast<int16_t*>(base + p.lds.off_coef);
    int32_t* ws = reinterpret_cast<int32_t*>(base + p.lds.off_ws);
    const jpeg::Geometry g = jpeg::geometry(p.H, p.W);
    const int mw = g.mcu_cols;
    const jpeg::SampleBuffers sb{base + p.lds.off_y, base + p.lds.off_c, mw};
    const size_t frame_bytes = (size_t)p.H * p.W * 3;
    const bool dwords = (p.W & 3) == 0 && (reinterpret_cast<uintptr_t>(p.dst) & 3) == 0;
    for (int i = blockIdx.x * jpeg::kDecodeWaves + wave; i < p.n; i += gridDim.x * jpeg::kDecodeWaves) {
        const int len = p.len[i];
        int st = jpeg::kSkipped;
        if (len > 0) {
            WindowFile f{p.files + p.off[i], len, base + p.lds.off_win, -2 * jpeg::kWindowBytes, lane};
            jpeg::FileHeader h;
            st = jpeg::parse_header(f, p.H, p.W, &h);
            if (st == jpeg::kDecoded) {
                wave_sync();                                           // (the tables of the file before this one have been read)
                jpeg::build_tables(f, h, T);
                wave_sync();
                uint8_t* dst = p.dst + (size_t)i * frame_bytes;
                jpeg::BitReader<WindowFile> r;
                r.start(&f, h.scan);
                // (scalars, not arrays indexed by the component: arrays indexed at run time would live in scratch memory)
                const jpeg::HuffTable* dc0 = &T->huff[h.td[0]]; const jpeg::HuffTable* dc1 = &T->huff[h.td[1]]; const jpeg::HuffTable* dc2 = &T->huff[h.td[2]];
                const jpeg::HuffTable* ac0 = &T->huff[2 + h.ta[0]]; const jpeg::HuffTable* ac1 = &T->huff[2 + h.ta[1]]; const jpeg::HuffTable* ac2 = &T->huff[2 + h.ta[2]];
                int pred0 = 0, pred1 = 0, pred2 = 0;
                for (int my = 0; my < g.mcu_rows && st == jpeg::kDecoded; ++my) {
                    for (int mx0 = 0; mx0 < mw && st == jpeg::kDecoded; mx0 += jpeg::kMcuGroup) {
                        const int gm = min(jpeg::kMcuGroup, mw - mx0), nb = gm * jpeg::kBlocksPerMcu;
                        for (int d = lane; d < nb * jpeg::kDecCoefStride / 2; d += 64) reinterpret_cast<uint32_t*>(coef)[d] = 0u;
                        wave_sync();
                        for (int b = 0; b < nb && st == jpeg::kDecoded; ++b) {      // the serial chain, the same in every lane
                            const int k = b % jpeg::kBlocksPerMcu;
                            int pred = k < 4 ? pred0 : k == 4 ? pred1 : pred2;
                            st = jpeg::decode_block(r, k < 4 ? *dc0 : k == 4 ? *dc1 : *dc2, k < 4 ? *ac0 : k == 4 ? *ac1 : *ac2, T->zz, &pred, coef + b * jpeg::kDecCoefStride);
                            if (k < 4) pred0 = pred; else if (k == 4) pred1 = pred; else pred2 = pred;
                        }
                        wave_sync();
                        if (st != jpeg::kDecoded) break;
                        for (int t0 = 0; t0 < nb * 8; t0 += 64) {                  // 8 blocks at a time: a column, then a row, per lane
                            const int t = t0 + lane, b = t >> 3, j = t & 7, k = b % jpeg::kBlocksPerMcu, c = k < 4 ? 0 : k - 3;
                            int32_t* w = ws + (b & 7) * jpeg::kWsBlockStride;
                            int32_t d[8];
                            if (t < nb * 8) {
                                const int16_t* cb = coef + b * jpeg::kDecCoefStride;
                                for (int row = 0; row < 8; ++row) d[row] = (int32_t)cb[row * 8 + j] * (int32_t)T->q[c][row * 8 + j];
                                jpeg::idct_pass(d, 11);
                                for (int row = 0; row < 8; ++row) w[row * jpeg::kWsRowStride + j] = d[row];
                            }
                            wave_sync();
                            if (t < nb * 8) {
                                for (int col = 0; col < 8; ++col) d[col] = w[j * jpeg::kWsRowStride + col];
                                jpeg::idct_pass(d, 18);
                                uint32_t lo4 = 0, hi4 = 0;
                                for (int col = 0; col < 4; ++col) {
                                    lo4 |= (uint32_t)jpeg::sample_of(d[col]) << (8 * col);
                                    hi4 |= (uint32_t)jpeg::sample_of(d[col + 4]) << (8 * col);
                                }
                                sb.store_block_row(my, mx0 + b / jpeg::kBlocksPerMcu, k, j, lo4, hi4);
                            }
                            wave_sync();
                        }
                    }
                    if (st == jpeg::kDecoded && my > 0) jpeg::output_mcu_row<64>(g, my - 1, sb, dst, lane, dwords);   // (the triangle filter reads the first chroma row of MCU row my)
                }
                if (st == jpeg::kDecoded) jpeg::output_mcu_row<64>(g, g.mcu_rows - 1, sb, dst, lane, dwords);
                wave_sync();                                           // the sample buffers are free for the next file
            }
        }
        if (lane == 0) p.status[i] = st;
    }
}

// the most LDS a workgroup of the handle's device may take (queried once per handle)
int lds_per_workgroup(trs_env* e, int* out)
{
    if (e->jpd_lds_max <= 0) {
        int v = 0;
        HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, e->device));
        int cu = 0;                                       // (a workgroup may take all of its CU's LDS, and some runtimes report only that figure in full)
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, e->device) == hipSuccess) v = std::max(v, cu);
        e->jpd_lds_max = v;
    }
    *out = e->jpd_lds_max;
    return TRS_OK;
}
}  // namespace

TRS_EXPORT int trs_decode_jpeg(trs_env* e, const uint8_t* d_files, const int64_t* d_off, const int32_t* d_len, int n_images, uint8_t* d_dst, int32_t* d_status)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (n_images < 1) return trs_internal_fail(TRS_ERR_ARG, "n_images < 1");
    if (!d_files || !d_off || !d_len) return trs_internal_fail(TRS_ERR_ARG, "null source");
    if (!d_dst || !d_status) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    if (e->H < 1 || e->W < 1) return trs_internal_fail(TRS_ERR_STATE, "the handle has no image size");
    HIPCHK(hipSetDevice(e->device));
    int lds_max = 0;
    int rc = lds_per_workgroup(e, &lds_max);
    if (rc) return rc;
    const jpeg::DecodeLds lds = jpeg::decode_lds(e->W);
    if (lds.total > lds_max || e->H > 65535 || e->W > 65535)
        return trs_internal_fail(TRS_ERR_LIMIT, "image too wide for the decoder: the sample rows of " + std::to_string(jpeg::kDecodeWaves) + " files in " + std::to_string(lds_max) +
                                                    " bytes of LDS allow img_w <= " + std::to_string(jpeg::decode_max_width(lds_max)));
    rc = trsim::quiesce_handle(e);
    if (rc) return rc;
    DecodeParams p{};
    p.files = d_files; p.off = d_off; p.len = d_len; p.dst = d_dst; p.status = d_status;
    p.n = n_images; p.H = e->H; p.W = e->W; p.lds = lds;
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(trs_jpeg_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds.total));
    const int grid = std::min((n_images + jpeg::kDecodeWaves - 1) / jpeg::kDecodeWaves, std::max(1, e->cu_count) * jpeg::kDecodeWgsPerCu);
    hipLaunchKernelGGL(trs_jpeg_decode_kernel, dim3(grid), dim3(64 * jpeg::kDecodeWaves), lds.total, e->sP, p);
    HIPCHK(hipGetLastError());
    trsim::resident_note_launch(e);                       // resident mode selected: this kernel has no completion flag, trs_sync waits for the stream
    return TRS_OK;
}

TRS_EXPORT int trs_decode_jpeg_host(trs_env* e, const uint8_t* h_blob, const int64_t* h_off, int n_images, uint8_t* h_dst, int32_t* h_status)
{
    if (!e) return trs_internal_fail(TRS_ERR_ARG, "null handle");
    if (n_images < 1) return trs_internal_fail(TRS_ERR_ARG, "n_images < 1");
    if (!h_blob || !h_off) return trs_internal_fail(TRS_ERR_ARG, "null source");
    if (!h_dst || !h_status) return trs_internal_fail(TRS_ERR_ARG, "null destination");
    const size_t n = (size_t)n_images;
    std::vector<int32_t> len(n);
    for (size_t i = 0; i < n; ++i) {
        const int64_t l = h_off[i + 1] - h_off[i];
        if (h_off[i] < 0 || l < 0 || l > INT32_MAX) return trs_internal_fail(TRS_ERR_ARG, "h_off must not decrease, and a file is shorter than 2 GiB");
        len[i] = (int32_t)l;
    }
    HIPCHK(hipSetDevice(e->device));
    const size_t blob_bytes = std::max<size_t>((size_t)h_off[n], 1), off_bytes = n * sizeof(int64_t), len_bytes = n * sizeof(int32_t);
    const size_t frame_bytes = (size_t)e->H * e->W * 3, dst_bytes = n * frame_bytes;
    if (e->jpd_files.bytes() < blob_bytes || e->jpd_meta.bytes() < off_bytes + 2 * len_bytes || e->jpd_dst.bytes() < dst_bytes) {
        int rc = trsim::quiesce_handle(e);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(e->sP));                              // what is replaced may still be in use
        hipError_t rh = e->jpd_files.reserve(blob_bytes);
        if (rh == hipSuccess) rh = e->jpd_meta.reserve(off_bytes + 2 * len_bytes);
        if (rh == hipSuccess) rh = e->jpd_dst.reserve(std::max<size_t>(dst_bytes, 4));
        if (rh != hipSuccess) return jpeg::no_memory(rh, blob_bytes + dst_bytes, "decoder scratch");
    }
    unsigned char* meta = e->jpd_meta.get();                              // offsets | lengths | statuses
    int64_t* d_off = reinterpret_cast<int64_t*>(meta);
    int32_t* d_len = reinterpret_cast<int32_t*>(meta + off_bytes);
    int32_t* d_status = reinterpret_cast<int32_t*>(meta + off_bytes + len_bytes);
    HIPCHK(hipStreamSynchronize(e->sP));                                  // (pageable copies below: the handle's earlier work on these buffers is done)
    HIPCHK(hipMemcpy(e->jpd_files.get(), h_blob, (size_t)h_off[n], hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off, h_off, off_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len, len.data(), len_bytes, hipMemcpyHostToDevice));
    trs_internal_count(e, 0, (size_t)h_off[n] + off_bytes + len_bytes);
    int rc = trs_decode_jpeg(e, e->jpd_files.get(), d_off, d_len, n_images, e->jpd_dst.get(), d_status);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->sP));
    HIPCHK(hipMemcpy(h_status, d_status, len_bytes, hipMemcpyDeviceToHost));
    // frames that were not written stay what the caller had: only decoded (and corrupt: undefined) frames are copied
    size_t copied = 0;
    for (size_t i = 0; i < n;) {
        if (h_status[i] != jpeg::kDecoded && h_status[i] != jpeg::kCorrupt) { ++i; continue; }
        size_t j = i + 1;
        while (j < n && (h_status[j] == jpeg::kDecoded || h_status[j] == jpeg::kCorrupt)) ++j;
        HIPCHK(hipMemcpy(h_dst + i * frame_bytes, e->jpd_dst.get() + i * frame_bytes, (j - i) * frame_bytes, hipMemcpyDeviceToHost));
        copied += (j - i) * frame_bytes;
        i = j;
    }
    trs_internal_count(e, len_bytes + copied, 0);
    return TRS_OK;
}
