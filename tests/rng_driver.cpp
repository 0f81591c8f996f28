// rng_driver.cpp -- prints what tamcmc-c_amd/csrc/rng.h computes on the CPU, for tests/test_rng.py:
//   kat   c0 c1 c2 c3 k0 k1 -> the four Philox4x32-10 words
//   u01   hi lo             -> the bits of u01_from_bits
//   addr  seed purpose chain iter idx -> the bits of rng_uniform2's pair and of rng_normal2's pair
//   clamp N                 -> u01_from_bits against the unclamped formula over N pseudo-random words and the 2^12 largest
// Arguments are read in that order, every command with its operands (integers in any C base).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../tamcmc-c_amd/csrc/rng.h"

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static uint64_t arg(char **argv, int &i) { return std::strtoull(argv[++i], nullptr, 0); }

// the formula before the clamp
static double u01_plain(uint64_t word) { return ((double)(word >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

int main(int argc, char **argv) {
    using namespace tamcmc;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "kat") && i + 6 < argc) {
            uint32_t v[6];
            for (int k = 0; k < 6; k++) v[k] = (uint32_t)arg(argv, i);
            const Philox4 r = philox4x32(v[0], v[1], v[2], v[3], v[4], v[5]);
            std::printf("kat %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", r.v[0], r.v[1], r.v[2], r.v[3]);
        } else if (!std::strcmp(argv[i], "u01") && i + 2 < argc) {
            const uint32_t hi = (uint32_t)arg(argv, i), lo = (uint32_t)arg(argv, i);
            std::printf("u01 %016" PRIx64 "\n", bits(u01_from_bits(hi, lo)));
        } else if (!std::strcmp(argv[i], "addr") && i + 5 < argc) {
            const uint64_t seed = arg(argv, i);
            const uint32_t purpose = (uint32_t)arg(argv, i), chain = (uint32_t)arg(argv, i);
            const uint64_t iter = arg(argv, i);
            const uint32_t idx = (uint32_t)arg(argv, i);
            double u0, u1, z0, z1;
            rng_uniform2(seed, purpose, chain, iter, idx, u0, u1);
            rng_normal2(seed, purpose, chain, iter, idx, z0, z1);
            std::printf("addr %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(u0), bits(u1), bits(z0), bits(z1));
        } else if (!std::strcmp(argv[i], "clamp") && i + 1 < argc) {
            const uint64_t n = arg(argv, i);
            uint64_t differ = 0, last_word = 0, outside = 0, tested = 0;
            auto one = [&](uint64_t w) {
                const double u = u01_from_bits((uint32_t)(w >> 32), (uint32_t)w);
                if (bits(u) != bits(u01_plain(w))) { differ++; last_word = w; }
                if (!(u > 0.0 && u < 1.0)) outside++;
                tested++;
            };
            for (uint64_t k = 0; k < n; k += 2) {  // Philox itself as the source of words
                const Philox4 r = philox4x32((uint32_t)k, (uint32_t)(k >> 32), 7u, 11u, 0x243F6A88u, 0x85A308D3u);
                one(((uint64_t)r.v[0] << 32) | r.v[1]);
                one(((uint64_t)r.v[2] << 32) | r.v[3]);
            }
            for (uint64_t j = 0; j < 4096; j++) one((((1ull << 53) - 1 - j) << 11) | 0x7ffull);  // the 2^12 largest 53-bit values
            one(0);
            std::printf("clamp tested %" PRIu64 " differ %" PRIu64 " last %016" PRIx64 " outside %" PRIu64 "\n", tested, differ, last_word, outside);
        } else {
            std::fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
    }
    return 0;
}
