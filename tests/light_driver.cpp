// Test driver (CPU): runs the PRODUCT's scene-lighting rule (triton-racer-sim_amd/csrc/trsim_tables.hpp, light_channel / light_colour — the code the
// kernels light palette entries with) on every channel value 0..255 for each (gain, bias) pair of a binary32 file, and writes the results out;
// tests/test_lighting_cpu.py builds it and compares them with a numpy restatement of include/trsim_spec.h ("scene lighting").
//   light_driver <pairs.bin> <out.bin>      pairs: float32 [n][2] (gain, bias); out: uint8 [n][256] by light_channel, then uint32 [n][256] by
//                                           light_colour on the grey colour x * 0x010101 with gains (g, g, g) and biases (b, b, b)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_tables.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> pairs;
    float v;
    while (std::fread(&v, 4, 1, f) == 1) pairs.push_back(v);
    std::fclose(f);
    const size_t n = pairs.size() / 2;
    std::vector<uint8_t> ch(n * 256);
    std::vector<uint32_t> col(n * 256);
    for (size_t i = 0; i < n; ++i) {
        const float g = pairs[2 * i], b = pairs[2 * i + 1];
        const float gb[8] = {g, g, g, 0.0f, b, b, b, 0.0f};
        for (uint32_t x = 0; x < 256; ++x) {
            ch[i * 256 + x] = (uint8_t)trsim::light_channel(x, g, b);
            col[i * 256 + x] = trsim::light_colour(x * 0x010101u, gb);
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 3;
    std::fwrite(ch.data(), 1, ch.size(), f);
    std::fwrite(col.data(), 4, col.size(), f);
    std::fclose(f);
    return 0;
}
