// tests/cpp/ratematch_host.cpp — the product's modem_ratematch_math.h on the host, for
// tests/test_ratematch_host.py (built there with the address and undefined-behaviour sanitizers):
//   ratematch_host rm <pattern as a string of 0 and 1> <cols> <nm> <out>
//     writes uint32 E, then for each m < nm uint32 pi(rank(m)), or 0xFFFFFFFF for a punctured m
//   ratematch_host crc <W> <poly> <init> <xorout> <nbits> <nframes> <stride> <in> <out>
//     reads nframes rows of `stride` bytes and writes the uint32 CRC of the first nbits of each,
//     computed as crc_kernel does: the registers of the 64 chunks, then six levels of joins in
//     which lane i takes the register of lane i + d (its own where there is none) and the powers
//     x^(d len) are squared from level to level.
#include "modem_ratematch_math.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool write_all(const char* path, const void* p, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

static uint32_t crc_as_the_kernel(const uint8_t* row, uint32_t L, uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout) {
    uint32_t xp[6];
    xp[0] = mk::crc_xpow(mk::crc_chunk_len(L), W, poly);
    for (int k = 1; k < 6; ++k) xp[k] = mk::crc_mul(xp[k - 1], xp[k - 1], W, poly);
    uint32_t v[mk::kCrcChunks];
    for (uint32_t l = 0; l < (uint32_t)mk::kCrcChunks; ++l)
        v[l] = mk::crc_chunk_reg(L, l, W, poly, init, [row](uint32_t i) { return (uint32_t)row[i]; });
    for (int k = 0; k < 6; ++k) {
        uint32_t next[mk::kCrcChunks];
        for (uint32_t l = 0; l < (uint32_t)mk::kCrcChunks; ++l) {
            const uint32_t src = l + (1u << k) < (uint32_t)mk::kCrcChunks ? l + (1u << k) : l;   // a shuffle down
            next[l] = mk::crc_join(v[l], v[src], xp[k], W, poly);
        }
        std::memcpy(v, next, sizeof v);
    }
    return v[0] ^ xorout;
}

int main(int argc, char** argv) {
    if (argc == 6 && !std::strcmp(argv[1], "rm")) {
        const uint32_t P = (uint32_t)std::strlen(argv[2]), C = (uint32_t)std::atoi(argv[3]), nm = (uint32_t)std::atoi(argv[4]);
        if (P < 1 || P > (uint32_t)mk::kRmMaxP || C < 1 || nm < 1) return 2;
        uint64_t mask = 0;
        for (uint32_t i = 0; i < P; ++i) mask |= (uint64_t)(argv[2][i] == '1') << i;
        const uint32_t w = mk::rm_popcount(mask), E = mk::rm_kept(mask, P, nm);
        if (w < 1 || E < 1) return 2;
        const uint32_t rows = mk::rm_rows(E, C), cl = E - (rows - 1) * C;
        std::vector<uint32_t> out(1 + (size_t)nm);
        out[0] = E;
        for (uint32_t m = 0; m < nm; ++m)
            out[1 + m] = mk::rm_is_kept(mask, P, m) ? mk::rm_pi(mk::rm_rank(mask, P, w, m), C, rows, cl) : 0xFFFFFFFFu;
        return write_all(argv[5], out.data(), out.size() * 4) ? 0 : 1;
    }
    if (argc == 11 && !std::strcmp(argv[1], "crc")) {
        const uint32_t W = (uint32_t)std::strtoul(argv[2], nullptr, 0), poly = (uint32_t)std::strtoul(argv[3], nullptr, 0);
        const uint32_t init = (uint32_t)std::strtoul(argv[4], nullptr, 0), xorout = (uint32_t)std::strtoul(argv[5], nullptr, 0);
        const uint32_t nbits = (uint32_t)std::atoi(argv[6]);
        const size_t nframes = (size_t)std::atoll(argv[7]), stride = (size_t)std::atoll(argv[8]);
        if ((W != 8 && W != 16 && W != 24 && W != 32) || nbits < 1 || stride < nbits) return 2;
        std::vector<uint8_t> in(nframes * stride);
        FILE* f = std::fopen(argv[9], "rb");
        if (!f) return 1;
        const size_t got = std::fread(in.data(), 1, in.size(), f);
        std::fclose(f);
        if (got != in.size()) return 1;
        std::vector<uint32_t> out(nframes);
        for (size_t r = 0; r < nframes; ++r) out[r] = crc_as_the_kernel(in.data() + r * stride, nbits, W, poly, init, xorout);
        return write_all(argv[10], out.data(), out.size() * 4) ? 0 : 1;
    }
    std::fprintf(stderr, "usage: ratematch_host rm <pattern> <cols> <nm> <out> | crc <W> <poly> <init> <xorout> <nbits> <nframes> <stride> <in> <out>\n");
    return 2;
}
