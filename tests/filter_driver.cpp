// Test driver (CPU): the host-only owner of the static colour filter (triton-racer-sim_amd/csrc/trsim_filter.hpp, the header alone) for
// tests/test_filter_cpu.py, which builds it with AddressSanitizer + UBSan.
//   filter_driver table                          the 512 entries of hsv_reciprocals, one per line
//   filter_driver filter <cfg> <in> <out>        <cfg>: the bytes of a trs_pre_config (refused by check_pre: its text on stderr, exit status 2);
//                                                <in>: colours as r g b bytes; <out>: filter_colour of each, as r g b bytes
#include <cstdio>
#include <cstring>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_filter.hpp"

static std::vector<unsigned char> slurp(const char* path)
{
    std::vector<unsigned char> v;
    if (FILE* f = std::fopen(path, "rb")) {
        unsigned char buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "table")) {
        int tab[512];
        trsim::hsv_reciprocals(tab);
        for (const int t : tab) std::printf("%d\n", t);
        return 0;
    }
    if (argc == 5 && !std::strcmp(argv[1], "filter")) {
        const std::vector<unsigned char> cb = slurp(argv[2]), in = slurp(argv[3]);
        trs_pre_config c;
        if (cb.size() != sizeof c || in.size() % 3) { std::fprintf(stderr, "bad input sizes\n"); return 1; }
        std::memcpy(&c, cb.data(), sizeof c);
        const char* why = nullptr;
        if (trsim::check_pre(&c, &why)) { std::fprintf(stderr, "%s\n", why); return 2; }
        std::vector<unsigned char> out(in.size());
        for (size_t i = 0; i < in.size(); i += 3) {
            const uint32_t o = trsim::filter_colour(c, (uint32_t)in[i] | ((uint32_t)in[i + 1] << 8) | ((uint32_t)in[i + 2] << 16));
            out[i] = (unsigned char)(o & 255u); out[i + 1] = (unsigned char)((o >> 8) & 255u); out[i + 2] = (unsigned char)((o >> 16) & 255u);
        }
        FILE* f = std::fopen(argv[4], "wb");
        if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 1; }
        std::fclose(f);
        return 0;
    }
    std::fprintf(stderr, "usage: filter_driver table | filter <cfg> <in> <out>\n");
    return 1;
}
