// tests/cpp/fec_host.cpp — the Viterbi decoder of include/modem_hip.h ("Convolutional code") on the
// CPU, from the very text the device kernels and the handle compile (rust-modem_amd/csrc/
// modem_fec_math.h: quantiser, predecessor, branch word, add-compare-select). No GPU. Built and run
// by tests/test_fec_host.py with the address and undefined-behaviour sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-unknown-pragmas
//       -I rust-modem_amd/csrc tests/cpp/fec_host.cpp -o fec_host
//   fec_host K TAIL NBITS NFRAMES STRIDE IN OUT G0 G1 [G2]
// IN: NFRAMES rows of STRIDE int8 LLRs (the first n * T of a row are used). OUT: NFRAMES * NBITS
// bytes, one decoded bit each, then NFRAMES int32 metrics. The decode time goes to stdout (the CPU
// baseline of tools/fec_rate.py, built there with -O2 and no sanitizer).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "modem_fec_math.h"

static bool decode_frame(const int8_t* llr, int K, const uint32_t* g, int n, bool tail, int nbits, uint8_t* out, int32_t* metric,
                         const std::vector<uint32_t>& table, std::vector<uint8_t>& dec, std::vector<int32_t>& pm,
                         std::vector<int32_t>& npm) {
    const uint32_t S = 1u << (K - 1);
    const int T = nbits + (tail ? K - 1 : 0);
    for (uint32_t s = 0; s < S; ++s) pm[s] = s ? mk::kFecStart : 0;
    for (int t = 0; t < T; ++t) {
        int32_t q[mk::kFecMaxN];
        for (int j = 0; j < n; ++j) q[j] = mk::fec_quant_i8(llr[(size_t)t * n + j]);
        for (uint32_t sn = 0; sn < S; ++sn) {
            int32_t m[2];
            for (uint32_t x = 0; x < 2; ++x) {
                m[x] = pm[mk::fec_pred(sn, x, K)];
                for (int j = 0; j < n; ++j) m[x] += mk::fec_branch_sign(table[sn], (int)x * mk::kFecMaxN + j) * q[j];
            }
            uint32_t x;
            npm[sn] = mk::fec_acs(m[0], m[1], x);
            dec[(size_t)t * S + sn] = (uint8_t)x;
        }
        pm.swap(npm);
    }
    uint32_t s = 0;
    if (!tail)
        for (uint32_t c = 1; c < S; ++c)
            if (pm[c] > pm[s]) s = c;
    *metric = pm[s];
    for (int t = T - 1; t >= 0; --t) {
        if (t < nbits) out[t] = (uint8_t)mk::fec_input_bit(s, K);
        s = mk::fec_pred(s, dec[(size_t)t * S + s], K);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 10 && argc != 11) {
        std::fprintf(stderr, "usage: fec_host K TAIL NBITS NFRAMES STRIDE IN OUT G0 G1 [G2]\n");
        return 2;
    }
    const int K = std::atoi(argv[1]), nbits = std::atoi(argv[3]), n = argc - 8;
    const bool tail = std::atoi(argv[2]) != 0;
    const size_t nframes = std::strtoull(argv[4], nullptr, 10), stride = std::strtoull(argv[5], nullptr, 10);
    uint32_t g[mk::kFecMaxN] = {0, 0, 0};
    for (int j = 0; j < n; ++j) g[j] = (uint32_t)std::strtoul(argv[8 + j], nullptr, 0);
    if (K < mk::kFecMinK || K > mk::kFecMaxK || nbits < 1) return 2;
    const int T = nbits + (tail ? K - 1 : 0);
    if (T > mk::fec_max_steps(K) || stride < (size_t)n * T) return 2;
    for (int j = 0; j < n; ++j)
        if (g[j] == 0 || g[j] >= (1u << K)) return 2;

    std::vector<int8_t> llr(nframes * stride);
    std::FILE* fi = std::fopen(argv[6], "rb");
    if (!fi || std::fread(llr.data(), 1, llr.size(), fi) != llr.size()) {
        std::fprintf(stderr, "fec_host: cannot read %zu bytes from %s\n", llr.size(), argv[6]);
        return 2;
    }
    std::fclose(fi);

    const uint32_t S = 1u << (K - 1);
    std::vector<uint32_t> table(S);
    for (uint32_t s = 0; s < S; ++s) table[s] = mk::fec_branch_word(s, K, g, n);
    std::vector<uint8_t> dec((size_t)T * S), out(nframes * (size_t)nbits);
    std::vector<int32_t> pm(S), npm(S), metric(nframes);
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t f = 0; f < nframes; ++f)
        decode_frame(llr.data() + f * stride, K, g, n, tail, nbits, out.data() + f * (size_t)nbits, &metric[f], table, dec, pm, npm);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::FILE* fo = std::fopen(argv[7], "wb");
    if (!fo || std::fwrite(out.data(), 1, out.size(), fo) != out.size() ||
        std::fwrite(metric.data(), sizeof(int32_t), metric.size(), fo) != metric.size()) {
        std::fprintf(stderr, "fec_host: cannot write %s\n", argv[7]);
        return 2;
    }
    std::fclose(fo);
    std::printf("decoded %zu frames of %d bits in %.6f s\n", nframes, nbits, sec);
    return 0;
}
