// rust-modem_amd/csrc/modem_fec.hip — the rate-1/n convolutional code (no reference counterpart;
// include/modem_hip.h, "Convolutional code"): a stateless encoder and a batched Viterbi decoder on
// the demapper's LLRs. The arithmetic that must agree with the host (quantiser, predecessor, branch
// word, add-compare-select) is modem_fec_math.h.
//
// conv_encode_kernel: a thread per (frame, step): the K bits of the register are read back from the
// frame's input bytes, the n parities stored. Not a hot path.
//
// viterbi_kernel<InT, N, R>: the wave is the unit, a workgroup is 1 .. 4 independent waves (as many
// as 64 KiB of LDS hold) and never meets at a barrier. A wave is a frame group:
//   S < 64   64 / S frames, lane = frame * S + state          (R = 1)
//   S = 64   one frame, lane = state                          (R = 1)
//   S > 64   one frame, lane l owns the R = S / 64 states i * 64 + l, i = 0 .. R-1
// Add-compare-select: the predecessors of state s' are the states 2 s' mod S and that + 1, so a lane
// fetches its two predecessor metrics by cross-lane shuffle from the lanes src0 = (frame base) |
// (2 lane mod min(S, 64)) and src0 | 1; for R > 1 the source slot is (2 i + (lane >> 5)) mod R, so
// every slot is shuffled once per x (2 R shuffles for 64 R states) and the lane's half picks between
// two of them. The branch metric is sum_j sign * q_j with the lane's 2 R N signs in registers (from
// the handle's branch-word table). One __ballot per slot and step is the decision word of all the
// wave's frames; lane 0 stores it to LDS at dec[t * R + i]: T * R words, at most 32 KiB.
// The quantised LLRs reach the step loop through LDS: the wave stages 256 frame-steps at a time
// (256 / frames steps of each of its frames, N bytes per step), consecutive lanes loading
// consecutive elements of a row; the loads of the next tile are issued before the step loop of the
// current one and land in 4 N registers, so no step waits on global memory. The step loop runs four
// steps per LDS read of N dwords (a broadcast within a frame).
// Traceback: lane f of the wave walks frame f back over the decision words (for R = 1 the word's
// address does not depend on the state, so the reads run ahead of the walk); the decoded bits of the
// wave's frames at step t are one ballot, stored over dec[t * R], and the whole wave then writes
// the rows out, 64 consecutive bytes per store.
//
// Plain vector stores only, no atomics, no global workspace, everything indexed at compile time: no
// scratch.
#include "modem_device.h"
#include "modem_fec_math.h"

namespace mk {

namespace {

constexpr int kEncNT = 256;
constexpr int kEncMaxBlocks = 2048;
constexpr int kVitMaxWaves = 4;                  // waves per workgroup, each a frame group of its own
constexpr int kVitTile = 256;                    // frame-steps a wave stages at a time
constexpr size_t kVitLds = 64 * 1024;            // LDS a workgroup may ask for

__global__ __launch_bounds__(kEncNT) void conv_encode_kernel(const ConvEncodeParams p) {
    const uint64_t total = p.nframes * p.T, stride = (uint64_t)gridDim.x * kEncNT;
    for (uint64_t idx = (uint64_t)blockIdx.x * kEncNT + threadIdx.x; idx < total; idx += stride) {
        const uint64_t f = idx / p.T, t = idx - f * p.T;
        const uint8_t* b = p.bits + f * p.in_stride;
        const uint32_t reg = fec_register(p.K, (int64_t)t, (int64_t)p.nbits, [b](int64_t i) { return (uint32_t)b[i]; });
        uint8_t* o = p.out + f * p.out_stride + t * (uint64_t)p.n;
        for (int j = 0; j < p.n; ++j) o[j] = (uint8_t)fec_coded_bit(reg, p.g[j]);
    }
}

// Element i of the LLR buffer, quantised.
template <typename T> struct VitIn;
template <> struct VitIn<int8_t> {
    __device__ static int32_t q(const void* p, uint64_t i, float) { return fec_quant_i8(static_cast<const int8_t*>(p)[i]); }
};
template <> struct VitIn<float> {
    __device__ static int32_t q(const void* p, uint64_t i, float qs) { return fec_quant_f32(static_cast<const float*>(p)[i], qs); }
};
template <> struct VitIn<__half> {
    __device__ static int32_t q(const void* p, uint64_t i, float qs) {
        return fec_quant_f32(__half2float(static_cast<const __half*>(p)[i]), qs);
    }
};

// LDS of one wave: T * R decision words, the final metrics of its 64 R states, one tile of quantised LLRs.
__host__ __device__ inline size_t vit_wave_bytes(int T, int R, int N) {
    return (size_t)T * R * 8 + 64 * R * 4 + (size_t)kVitTile * N;
}

// The wave's own LDS traffic: what one lane stored, another lane of the wave may read afterwards.
__device__ __forceinline__ void vit_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename InT, int N, int R>
__global__ __launch_bounds__(64 * kVitMaxWaves) void viterbi_kernel(const ViterbiParams p) {
    extern __shared__ uint64_t vit_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = p.K, T = p.T;
    const int lS = K - 1, lSm = lS < 6 ? lS : 6;        // log2 of the states, and of those a wave holds per frame and slot
    const int lF = 6 - lSm, F = 1 << lF;                // frames per wave
    const int Sm = 1 << lSm;
    const uint64_t f0 = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave) << lF;
    if (f0 >= p.nframes) return;                        // the whole wave: no barrier follows
    char* base = reinterpret_cast<char*>(vit_lds) + wave * vit_wave_bytes(T, R, N);
    uint64_t* dec = reinterpret_cast<uint64_t*>(base);
    int32_t* pmf = reinterpret_cast<int32_t*>(base + (size_t)T * R * 8);
    int8_t* qt = reinterpret_cast<int8_t*>(pmf + 64 * R);

    // lane f < F: frame f0 + f exists and is to be decoded
    bool mine = false;
    if (lane < F && f0 + lane < p.nframes) mine = !p.ok || p.ok[f0 + lane] != 0;
    const uint64_t vmask = __ballot(mine);
    int32_t met = 0;

    if (vmask) {
        const int lTS = 8 - lF, TS = 1 << lTS;          // steps of each frame per tile: 256 / F
        const int ntiles = (T + TS - 1) >> lTS;
        const int64_t ncoded = (int64_t)N * T;
        // element e = i * 64 + lane of a tile: frame e / (TS N), offset e mod (TS N) in the tile's part of its row
        auto load_tile = [&](int tile, int32_t(&r)[4 * N]) {
#pragma unroll
            for (int i = 0; i < 4 * N; ++i) {
                const int e = i * 64 + lane;
                const int fi = (e >> lTS) / N;
                const int64_t col = (int64_t)tile * (TS * N) + (e - fi * (TS * N));
                int32_t q = 0;
                if (((vmask >> fi) & 1) && col < ncoded) q = VitIn<InT>::q(p.llr, (f0 + fi) * p.stride + (uint64_t)col, p.qscale);
                r[i] = q;
            }
        };
        int32_t r[4 * N];
        load_tile(0, r);

        const int s_lane = lane & (Sm - 1);
        int32_t sg[R][2][N], pm[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const uint32_t w = p.table[i * 64 + s_lane];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int j = 0; j < N; ++j) sg[i][x][j] = fec_branch_sign(w, x * kFecMaxN + j);
            pm[i] = i * 64 + s_lane == 0 ? 0 : kFecStart;
        }
        const int src0 = (lane & ~(Sm - 1)) | ((lane << 1) & (Sm - 1));
        const int32_t upper = R > 1 && (lane & 32) ? -1 : 0;   // all ones: the lane's predecessors sit in the odd slot
        const int8_t* qrow = qt + (lane >> lSm) * (TS * N);

        for (int tile = 0; tile < ntiles; ++tile) {
            vit_wave_sync();                            // the reads of the previous tile are done
#pragma unroll
            for (int i = 0; i < 4 * N; ++i) qt[i * 64 + lane] = (int8_t)r[i];
            vit_wave_sync();
            if (tile + 1 < ntiles) load_tile(tile + 1, r);
            const int t0 = tile << lTS, tn = T - t0 < TS ? T - t0 : TS;
            for (int tt = 0; tt < tn; tt += 4) {
                uint32_t w[N];
#pragma unroll
                for (int k = 0; k < N; ++k) w[k] = *reinterpret_cast<const uint32_t*>(qrow + tt * N + 4 * k);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (tt + u < tn) {                  // wave-uniform
                        int32_t q[N];
#pragma unroll
                        for (int j = 0; j < N; ++j) {
                            const int b = u * N + j;
                            q[j] = (int32_t)(int8_t)(w[b >> 2] >> (8 * (b & 3)));
                        }
                        int32_t v0[R], v1[R];
#pragma unroll
                        for (int k = 0; k < R; ++k) {
                            v0[k] = __shfl(pm[k], src0, 64);
                            v1[k] = __shfl(pm[k], src0 | 1, 64);
                        }
#pragma unroll
                        for (int i = 0; i < R; ++i) {
                            int32_t b0 = 0, b1 = 0;
#pragma unroll
                            for (int j = 0; j < N; ++j) {
                                b0 += __mul24(sg[i][0][j], q[j]);
                                b1 += __mul24(sg[i][1][j], q[j]);
                            }
                            const int k0 = (2 * i) % R, k1 = (2 * i + 1) % R;
                            // a bitwise select: `upper ? v[k1] : v[k0]` becomes a runtime-indexed array in scratch
                            const int32_t a0 = (v0[k1] & upper) | (v0[k0] & ~upper);
                            const int32_t a1 = (v1[k1] & upper) | (v1[k0] & ~upper);
                            uint32_t x;
                            pm[i] = fec_acs(a0 + b0, a1 + b1, x);
                            const uint64_t word = __ballot(x != 0);
                            if (lane == 0) dec[(size_t)(t0 + tt + u) * R + i] = word;
                        }
                    }
                }
            }
        }

#pragma unroll
        for (int i = 0; i < R; ++i) pmf[i * 64 + lane] = pm[i];
        vit_wave_sync();
        if (lane < F) {                                 // every frame of the wave, decoded or not: lane 0 stores
            const int fb = lane << lSm;                 // the frame's first lane (0 for one frame per wave)
            uint32_t s = 0;
            if (!p.tail) {
                int32_t best = pmf[fb];
                for (uint32_t c = 1; c < (1u << lS); ++c) {
                    const int32_t v = pmf[fb + c];
                    if (v > best) { best = v; s = c; }
                }
            }
            met = pmf[fb + s];
            for (int t = T - 1; t >= 0; --t) {
                const uint64_t w = dec[(size_t)t * R + (R > 1 ? s >> 6 : 0)];
                const uint32_t x = (uint32_t)(w >> (fb + (s & 63))) & 1u;
                const uint32_t bit = fec_input_bit(s, K);
                s = fec_pred(s, x, K);
                const uint64_t bits = __ballot(bit != 0);   // bit f: frame f's information bit t
                if (lane == 0) dec[(size_t)t * R] = bits;
            }
        }
        vit_wave_sync();
    }

    for (int fi = 0; fi < F; ++fi) {
        const uint64_t f = f0 + fi;
        if (f >= p.nframes) break;
        const bool valid = (vmask >> fi) & 1;
        uint8_t* o = p.out + f * p.out_stride;
        for (int t = lane; t < p.nbits; t += 64)
            o[t] = valid ? (uint8_t)((reinterpret_cast<const uint32_t*>(dec)[2 * (size_t)t * R] >> fi) & 1u) : (uint8_t)0;
    }
    if (p.metric && lane < F && f0 + lane < p.nframes) p.metric[f0 + lane] = mine ? met : 0;
}

template <typename InT, int N>
hipError_t viterbi_go(const ViterbiParams& p, hipStream_t s) {
    const int lS = p.K - 1, R = lS > 6 ? 1 << (lS - 6) : 1, lF = lS < 6 ? 6 - lS : 0;
    const size_t wb = vit_wave_bytes(p.T, R, N);
    const uint64_t groups = (p.nframes + ((uint64_t)1 << lF) - 1) >> lF;
    uint64_t waves = kVitLds / wb;
    waves = waves < 1 ? 1 : waves > kVitMaxWaves ? kVitMaxWaves : waves;
    if (waves > groups) waves = groups;
    const uint64_t blocks = (groups + waves - 1) / waves;
    if (wb > kVitLds || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block((unsigned)(64 * waves));
    const size_t lds = wb * waves;
    switch (R) {
    case 1: hipLaunchKernelGGL((viterbi_kernel<InT, N, 1>), grid, block, lds, s, p); break;
    case 2: hipLaunchKernelGGL((viterbi_kernel<InT, N, 2>), grid, block, lds, s, p); break;
    default: hipLaunchKernelGGL((viterbi_kernel<InT, N, 4>), grid, block, lds, s, p); break;
    }
    return hipGetLastError();
}

template <typename InT>
hipError_t viterbi_n(const ViterbiParams& p, hipStream_t s) {
    return p.n == 2 ? viterbi_go<InT, 2>(p, s) : viterbi_go<InT, 3>(p, s);
}

}  // namespace

hipError_t launch_conv_encode(const ConvEncodeParams& p, hipStream_t s) {
    if (p.K < kFecMinK || p.K > kFecMaxK || p.n < 2 || p.n > kFecMaxN || p.nbits == 0 || p.T < p.nbits ||
        p.T - p.nbits > (uint64_t)(p.K - 1) || p.in_stride < p.nbits || p.out_stride / (uint64_t)p.n < p.T)
        return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.bits || !p.out || p.nframes > ~(uint64_t)0 / p.T) return hipErrorInvalidValue;
    const uint64_t nblk = (p.nframes * p.T + kEncNT - 1) / kEncNT;
    hipLaunchKernelGGL(conv_encode_kernel, dim3((unsigned)(nblk < (uint64_t)kEncMaxBlocks ? nblk : (uint64_t)kEncMaxBlocks)),
                       dim3(kEncNT), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_viterbi(const ViterbiParams& p, int in_dtype, hipStream_t s) {
    if (p.K < kFecMinK || p.K > kFecMaxK || p.n < 2 || p.n > kFecMaxN || p.nbits < 1 ||
        p.T != p.nbits + (p.tail ? p.K - 1 : 0) || p.T > fec_max_steps(p.K) || p.stride < (uint64_t)p.n * (uint64_t)p.T ||
        p.out_stride < (uint64_t)p.nbits)
        return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.llr || !p.out || !p.table) return hipErrorInvalidValue;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p.llr);
    switch (in_dtype) {
    case 0: return a % 4 ? hipErrorInvalidValue : viterbi_n<float>(p, s);
    case 1: return a % 2 ? hipErrorInvalidValue : viterbi_n<__half>(p, s);
    case 3: return viterbi_n<int8_t>(p, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mk
