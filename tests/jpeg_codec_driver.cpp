// Drives csrc/trsim_jpeg_codec.hpp on the host (tests/test_jpeg_codec_cpu.py builds this file with the address and undefined-behaviour sanitizers).
//   jpeg_codec_driver frame <H> <W> <quality> <file>   codec_frame of the uint8[H][W][3] frame in <file>: one line, the frame as hex
//   jpeg_codec_driver plan <W>                         the kernel's LDS plan: the offsets and the total | the width limit at 160 KiB
// Source and destination are heap buffers of exactly the frame's size, so that a read or write beyond either is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../triton-racer-sim_amd/csrc/trsim_jpeg_codec.hpp"

using namespace trsim::jpeg;

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    if (!std::strcmp(argv[1], "plan")) {
        const CodecLds l = codec_lds(std::atoi(argv[2]));
        std::printf("%d %d %d %d %d %d %d %d\n%d\n", l.off_q, l.off_raw, l.off_y, l.off_c, l.off_ws, l.off_yout, l.off_cring, l.total, codec_max_width(kMaxLdsBytes));
        return 0;
    }
    if (std::strcmp(argv[1], "frame") || argc < 6) return 2;
    const int H = std::atoi(argv[2]), W = std::atoi(argv[3]), q = std::atoi(argv[4]);
    if (H < 1 || W < 1) return 2;
    const size_t bytes = (size_t)H * W * 3;
    uint8_t* src = static_cast<uint8_t*>(std::malloc(bytes));
    uint8_t* dst = static_cast<uint8_t*>(std::malloc(bytes));
    FILE* f = std::fopen(argv[5], "rb");
    if (!src || !dst || !f || std::fread(src, 1, bytes, f) != bytes) return 4;
    std::fclose(f);
    std::memset(dst, 0xA5, bytes);
    const bool ok = codec_frame(H, W, q, src, dst);
    if (ok) {
        for (size_t i = 0; i < bytes; ++i) std::printf("%02x", dst[i]);
        std::printf("\n");
    }
    std::free(src);
    std::free(dst);
    return ok ? 0 : 3;
}
