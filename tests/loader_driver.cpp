// Test driver (CPU): the rules of the training minibatches (triton-racer-sim_amd/csrc/trsim_loader.hpp — the header alone) printed for
// tests/test_loader_cpu.py, which builds it with AddressSanitizer + UBSan and compares it with Python statements of the rules.
//   loader_driver defaults                                                                   the default config, one "name value" per line
//   loader_driver config <loader> <label> <layout> <dtype> <n_records> <n_train> <struct_size delta>      "ok" or the refusal's text
//   loader_driver range <n_records> <n_train> <split> <epoch> <first> <count>                "ok" or the refusal's text
//   loader_driver call <loader> <render: 0 | 1> <frames> <rows> <images> <features> <labels> <index>      "ok" or the refusal's text
//        per pointer 0: NULL, 1: aligned, 2: off its alignment (images: 16-byte aligned + 4; the others: 4-byte aligned + 2)
//   loader_driver perm <key> <n>                                                             perm(key, n, i) for i = 0 .. n - 1, one per line
//   loader_driver order <seed> <n_records> <n_train> <split> <epoch>                         the record at every position of the split, one per line
//   loader_driver unit255                                                                    (float)v / 255 for v = 0 .. 255 as the kernel computes it, bit patterns
//   loader_driver sample <loader> <label> <file of float32 [n][8] rows>                      per row "<F> feat0 feat1 label0 label1" as bit patterns (8 hex digits)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../triton-racer-sim_amd/csrc/trsim_loader.hpp"

using namespace trsim;

static uint32_t bits_of(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "defaults")) {
        trs_loader_config c;
        loader_defaults(&c);
        std::printf("struct_size %u\nloader %d\nlabel %d\nlayout %d\ndtype %d\nn_records %d\nn_train %d\nseed %llu\n", c.struct_size, c.loader, c.label, c.layout,
                    c.dtype, c.n_records, c.n_train, (unsigned long long)c.seed);
        return 0;
    }
    if (!std::strcmp(argv[1], "config") && argc == 9) {
        trs_loader_config c;
        loader_defaults(&c);
        c.loader = std::atoi(argv[2]); c.label = std::atoi(argv[3]); c.layout = std::atoi(argv[4]); c.dtype = std::atoi(argv[5]);
        c.n_records = std::atoi(argv[6]); c.n_train = std::atoi(argv[7]);
        c.struct_size += (uint32_t)std::atoi(argv[8]);
        const char* why = loader_config_error(&c);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (!std::strcmp(argv[1], "range") && argc == 8) {
        trs_loader_config c;
        loader_defaults(&c);
        c.n_records = std::atoi(argv[2]); c.n_train = std::atoi(argv[3]);
        if (loader_config_error(&c)) return 2;
        const char* why = loader_range_error(&c, std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (!std::strcmp(argv[1], "call") && argc == 10) {
        alignas(16) static unsigned char room[6][32];
        trs_loader_config c;
        loader_defaults(&c);
        c.loader = std::atoi(argv[2]);
        if (loader_config_error(&c)) return 2;
        const void* ptr[6];
        for (int k = 0; k < 6; ++k) {
            const int how = std::atoi(argv[4 + k]);
            ptr[k] = how == 0 ? nullptr : room[k] + (how == 1 ? 0 : k == 2 ? 4 : 2);
        }
        const LoaderCall call{ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], ptr[5], std::atoi(argv[3]) != 0};
        const char* why = loader_call_error(&c, call);
        std::printf("%s\n", why ? why : "ok");
        return 0;
    }
    if (!std::strcmp(argv[1], "perm") && argc == 4) {
        const uint64_t key = std::strtoull(argv[2], nullptr, 0);
        const uint32_t n = (uint32_t)std::strtoul(argv[3], nullptr, 0);
        for (uint32_t i = 0; i < n; ++i) std::printf("%u\n", perm(key, n, i));
        return 0;
    }
    if (!std::strcmp(argv[1], "order") && argc == 7) {
        trs_loader_config c;
        loader_defaults(&c);
        c.seed = std::strtoull(argv[2], nullptr, 0); c.n_records = std::atoi(argv[3]); c.n_train = std::atoi(argv[4]);
        const int split = std::atoi(argv[5]), epoch = std::atoi(argv[6]);
        if (loader_config_error(&c) || loader_range_error(&c, split, epoch, 0, 0)) return 2;
        const Order o = Order::of(c.seed, c.n_records, c.n_train, split, epoch);
        for (uint32_t p = 0; p < o.n_s; ++p) std::printf("%u\n", o.record(p));
        return 0;
    }
    if (!std::strcmp(argv[1], "unit255")) {
        for (uint32_t v = 0; v < 256; ++v) std::printf("%08x\n", bits_of(unit255(v)));
        return 0;
    }
    if (!std::strcmp(argv[1], "sample") && argc == 5) {
        FILE* f = std::fopen(argv[4], "rb");
        if (!f) return 2;
        std::vector<float> rows;
        float row[kLoaderRowFloats];
        while (std::fread(row, sizeof row, 1, f) == 1) rows.insert(rows.end(), row, row + kLoaderRowFloats);
        std::fclose(f);
        const int loader = std::atoi(argv[2]), label = std::atoi(argv[3]);
        for (size_t r = 0; r < rows.size() / kLoaderRowFloats; ++r) {
            const Sample s = row_to_sample(&rows[r * kLoaderRowFloats], loader, label);
            std::printf("%d %08x %08x %08x %08x\n", loader_features(loader), bits_of(s.feat[0]), bits_of(s.feat[1]), bits_of(s.label[0]), bits_of(s.label[1]));
        }
        return 0;
    }
    return 2;
}
