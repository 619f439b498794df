// rust-modem_amd/csrc/modem_noncoh.hip — noncoherent receivers for the phasors that carry state
// from symbol to symbol (no reference counterpart: the reference's Demodulator ends at I/Q).
//
// diff  (DMPSK, dmpsk.rs:29-33)  z[k] = r[k] * conj(r[k-1]),  c(s) = z.re*tab[2s] + z.im*tab[2s+1]
// fsk   (MFSK mfsk.rs:60-75, BFSK bfsk.rs:23-55)
//                                S[k,m] = sum_{i<sps} x[k*sps+i] * e^{-j omega[m] i},  E = |S|^2
// both  sym = argmax of the metric (lowest index on ties),
//       llr[k*bps + j] = scale * (max_{bit_j=0} metric - max_{bit_j=1} metric),  j = 0 the MSB.
//
// The maxima of a bit are gathered over the binary tree of the symbol index, as modem_demap.hip
// gathers its minima (max is exact too); the tree also hands the arg max upwards, the left child
// winning a tie. Every array is indexed at compile time: no scratch.
//
// diff: one lane per symbol, a grid-stride loop, the table in LDS (a broadcast read). A lane
// loads its own point and the one before it (the first lane of a call: the handle's carried
// point), so workgroup and call boundaries need nothing else.
//
// fsk: a workgroup takes a tile of NS symbols. A wave holds 64 symbols (one per lane) and one
// group of TM <= 16 tones: 2 * TM accumulators per lane. The samples go through LDS in chunks of
// at most IC samples per symbol (coalesced rows in, one ds_read_b64 per lane and sample out; the
// odd row stride keeps the 64 lanes on distinct banks); the twiddles of a (group, sample) are
// wave-uniform and contiguous, so they arrive by scalar loads and sit in SGPRs: 4 * TM FMAs per
// LDS read. A symbol's samples are summed in ascending order whatever the call boundaries are.
// The energies then go to LDS (row stride 2^bps + 1), where one lane per symbol runs the tree
// and all lanes copy the rows out.
//   tones  waves  symbols/tile  IC   LDS
//   <= 16    4       256        16   34 KiB
//     32     4       128        32   33 KiB
//     64     4        64        64   33 KiB
//    128     8        64        64   33 KiB
//    256    16        64        64   64 KiB (the energies)
#include "modem_device.h"
#include "modem_llr_store.h"

namespace mk {

namespace {

// max over the indices [base, base + 2^L) and its lowest arg max; the bits of weight < 2^L
// update their maxima (bit of weight 2^(L-1) is j = NB - L, MSB first).
template <int L, int NB, typename Leaf>
__device__ __forceinline__ float noncoh_tree(const Leaf& leaf, int base, float (&m0)[NB], float (&m1)[NB], int& arg) {
    if constexpr (L == 0) {
        arg = base;
        return leaf(base);
    } else {
        int ia, ib;
        const float a = noncoh_tree<L - 1, NB>(leaf, base, m0, m1, ia);
        const float b = noncoh_tree<L - 1, NB>(leaf, base + (1 << (L - 1)), m0, m1, ib);
        m0[NB - L] = __builtin_fmaxf(m0[NB - L], a);
        m1[NB - L] = __builtin_fmaxf(m1[NB - L], b);
        arg = a >= b ? ia : ib;
        return a >= b ? a : b;
    }
}

// The decision and the NB LLRs of one symbol, stored (either output may be null). Above 16
// values the tree covers the low 4 bits and a rolled loop walks the 2^(NB-4) subtrees in
// ascending order (a strictly greater subtree maximum takes the arg max: the lowest index still
// wins a tie), so that no more than 16 metrics are live at once.
template <int NB, typename OutT, typename Leaf>
__device__ __forceinline__ void noncoh_decide(const Leaf& leaf, float scale, int64_t k, uint8_t* sym, void* llr, int vw) {
    constexpr int LB = NB < 4 ? NB : 4, HB = NB - LB;
    float m0[NB], m1[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) m0[j] = m1[j] = -__builtin_inff();
    float best = -__builtin_inff();
    int arg = 0;
#pragma unroll 1
    for (int u = 0; u < (1 << HB); ++u) {
        int a;
        const float v = noncoh_tree<LB, NB>(leaf, u << LB, m0, m1, a);
#pragma unroll
        for (int j = 0; j < HB; ++j) {                    // bit j of the index is bit HB-1-j of u
            const bool one = (u >> (HB - 1 - j)) & 1;
            m0[j] = one ? m0[j] : __builtin_fmaxf(m0[j], v);
            m1[j] = one ? __builtin_fmaxf(m1[j], v) : m1[j];
        }
        if (v > best || u == 0) { best = v; arg = a; }
    }
    if (sym) sym[k] = (uint8_t)arg;
    if (llr) {
        float v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) v[j] = scale * (m0[j] - m1[j]);
        demap_put<OutT, NB>(static_cast<char*>(llr) + k * (NB * DemapOut<OutT>::esz), v, vw);
    }
}

// Sample idx of an interleaved (i, q) buffer, widened to f32; pair: naturally aligned pairs.
template <typename InT>
__device__ __forceinline__ float2 load_iq(const void* base, int64_t idx, int pair);
template <>
__device__ __forceinline__ float2 load_iq<float>(const void* base, int64_t idx, int pair) {
    const float* x = static_cast<const float*>(base) + 2 * idx;
    if (pair) return *reinterpret_cast<const float2*>(x);
    return make_float2(x[0], x[1]);
}
template <>
__device__ __forceinline__ float2 load_iq<__half>(const void* base, int64_t idx, int pair) {
    const __half* x = static_cast<const __half*>(base) + 2 * idx;
    if (pair) {
        const __half2 v = *reinterpret_cast<const __half2*>(x);
        return make_float2(__low2float(v), __high2float(v));
    }
    return make_float2(__half2float(x[0]), __half2float(x[1]));
}

// ------------------------------------------------------------------------------- diff ----
constexpr int kDiffNT = 256;
constexpr int kDiffMaxBlocks = 2048;   // 8 workgroups per CU; the rest by the grid-stride loop

struct LeafCorr {
    const float* tab; float re, im;
    __device__ __forceinline__ float operator()(int s) const {
        return __builtin_fmaf(im, tab[2 * s + 1], re * tab[2 * s]);
    }
};

template <int BPS, typename InT, typename OutT>
__global__ __launch_bounds__(kDiffNT) void diff_kernel(const DiffParams p, int pair, int vw) {
    __shared__ __attribute__((aligned(16))) float tab[2 << BPS];
    for (int i = threadIdx.x; i < (2 << BPS); i += kDiffNT) tab[i] = p.tab[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kDiffNT;
    for (int64_t k = (int64_t)blockIdx.x * kDiffNT + threadIdx.x; k < p.nsym; k += stride) {
        const float2 r = load_iq<InT>(p.iq, k, pair);
        const float2 q = k ? load_iq<InT>(p.iq, k - 1, pair) : *p.prev;
        if (k == p.nsym - 1) *p.prev_new = r;
        const float zre = __builtin_fmaf(r.y, q.y, r.x * q.x);
        const float zim = __builtin_fmaf(r.y, q.x, -(r.x * q.y));
        noncoh_decide<BPS, OutT>(LeafCorr{tab, zre, zim}, p.scale, k, p.sym, p.llr, vw);
    }
}

template <int BPS, typename InT, typename OutT>
hipError_t diff_go(const DiffParams& p, hipStream_t s) {
    const int vw = p.llr ? demap_store_width(p.llr, BPS * DemapOut<OutT>::esz) : 1;
    if (vw < DemapOut<OutT>::esz) return hipErrorInvalidValue;              // not even element-aligned
    const uintptr_t in = reinterpret_cast<uintptr_t>(p.iq);
    if (in % sizeof(InT)) return hipErrorInvalidValue;
    const int pair = in % (2 * sizeof(InT)) == 0;
    const int64_t nblk = (p.nsym + kDiffNT - 1) / kDiffNT;
    hipLaunchKernelGGL((diff_kernel<BPS, InT, OutT>), dim3((unsigned)(nblk < kDiffMaxBlocks ? nblk : kDiffMaxBlocks)),
                       dim3(kDiffNT), 0, s, p, pair, vw);
    return hipGetLastError();
}

template <int BPS, typename InT>
hipError_t diff_out(const DiffParams& p, int out_dtype, hipStream_t s) {
    switch (out_dtype) {
    case 0: return diff_go<BPS, InT, float>(p, s);
    case 1: return diff_go<BPS, InT, __half>(p, s);
    case 3: return diff_go<BPS, InT, int8_t>(p, s);
    default: return hipErrorInvalidValue;
    }
}

template <int BPS>
hipError_t diff_in(const DiffParams& p, int in_dtype, int out_dtype, hipStream_t s) {
    switch (in_dtype) {
    case 0: return diff_out<BPS, float>(p, out_dtype, s);
    case 1: return diff_out<BPS, __half>(p, out_dtype, s);
    default: return hipErrorInvalidValue;
    }
}

// -------------------------------------------------------------------------------- fsk ----
template <int BPS> struct FskShape {
    static constexpr int M = 1 << BPS;
    static constexpr int TM = M < kFskTM ? M : kFskTM;   // tones per wave
    static constexpr int G = M / TM;                     // tone groups
    static constexpr int NW = G < 4 ? 4 : G;             // waves per workgroup, one group each
    static constexpr int NT = 64 * NW;
    static constexpr int NSET = NW / G;                  // sets of 64 symbols per tile
    static constexpr int NS = 64 * NSET;
    static constexpr int IC = 64 / NSET;                 // samples per symbol and chunk
    static constexpr int XROW = IC + 1;                  // odd: lane * XROW + c covers 32 banks twice
    static constexpr int EROW = M + 1;
    static constexpr int XBYTES = NS * XROW * 8, EBYTES = NS * EROW * 4;
    static constexpr int LDS = XBYTES > EBYTES ? XBYTES : EBYTES;
};

struct LeafLds {
    const float* e;
    __device__ __forceinline__ float operator()(int m) const { return e[m]; }
};

// Sample j of the logical stream: the carried samples, then this call's.
template <typename InT>
__device__ __forceinline__ float2 fsk_sample(const FskParams& p, int64_t j, int pair_in, int pair_carry) {
    return j < p.ncarry ? load_iq<InT>(p.carry, j, pair_carry) : load_iq<InT>(p.in, j - p.ncarry, pair_in);
}

template <int BPS, typename InT, typename OutT>
__global__ __launch_bounds__(FskShape<BPS>::NT) void fsk_kernel(const FskParams p, int pair_in, int vw) {
    using S = FskShape<BPS>;
    constexpr int M = S::M, TM = S::TM, G = S::G;
    __shared__ __attribute__((aligned(16))) char lds[S::LDS];
    float2* xs = reinterpret_cast<float2*>(lds);
    float* es = reinterpret_cast<float*>(lds);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wave % G, srow = (wave / G) * 64 + lane;
    const int sps = p.sps;
    const int64_t k0 = (int64_t)blockIdx.x * S::NS;
    const int nrow = (int)(p.nsym - k0 < S::NS ? p.nsym - k0 : S::NS);

    float2 acc[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) acc[t] = make_float2(0.f, 0.f);

    for (int i0 = 0; i0 < sps; i0 += S::IC) {
        const int ic = sps - i0 < S::IC ? sps - i0 : S::IC;
        const float inv_ic = 1.0f / (float)ic;
        __syncthreads();                                  // the previous chunk has been read
        for (int idx = tid; idx < nrow * ic; idx += S::NT) {
            // idx = r * ic + c: the estimate of r is off by at most one (idx < 2^14)
            int r = (int)(((float)idx + 0.5f) * inv_ic);
            int c = idx - r * ic;
            if (c < 0) { --r; c += ic; } else if (c >= ic) { ++r; c -= ic; }
            xs[r * S::XROW + c] = fsk_sample<InT>(p, (k0 + r) * sps + i0 + c, pair_in, 1);
        }
        __syncthreads();
        const float2* __restrict__ tw = p.tw + ((size_t)g * sps + i0) * TM;
        const float2* xrow = xs + srow * S::XROW;
#pragma unroll 2
        for (int c = 0; c < ic; ++c) {
            const float2 x = xrow[c];
#pragma unroll
            for (int t = 0; t < TM; ++t) {
                const float2 w = tw[c * TM + t];
                acc[t].x = __builtin_fmaf(-x.y, w.y, __builtin_fmaf(x.x, w.x, acc[t].x));
                acc[t].y = __builtin_fmaf(x.y, w.x, __builtin_fmaf(x.x, w.y, acc[t].y));
            }
        }
    }
    __syncthreads();                                      // the samples are done with: energies over them
#pragma unroll
    for (int t = 0; t < TM; ++t)
        es[srow * S::EROW + g * TM + t] = __builtin_fmaf(acc[t].y, acc[t].y, acc[t].x * acc[t].x);
    __syncthreads();
    if (tid < nrow && (p.sym || p.llr))
        noncoh_decide<BPS, OutT>(LeafLds{es + tid * S::EROW}, p.scale, k0 + tid, p.sym, p.llr, vw);
    if (p.energy) {
        float* e = p.energy + k0 * M;
        for (int idx = tid; idx < nrow * M; idx += S::NT) e[idx] = es[(idx >> BPS) * S::EROW + (idx & (M - 1))];
    }
}

// The samples after the last whole symbol, raw, into the handle's other carry buffer.
template <typename InT>
__global__ __launch_bounds__(256) void fsk_carry_kernel(const FskParams p) {
    const int64_t first = p.nsym * p.sps, count = p.ncarry + p.n - first;
    const InT* c = static_cast<const InT*>(p.carry);
    const InT* x = static_cast<const InT*>(p.in);
    InT* d = static_cast<InT*>(p.carry_new);
    for (int64_t i = threadIdx.x; i < count; i += 256) {
        const int64_t j = first + i;
        const InT* src = j < p.ncarry ? c + 2 * j : x + 2 * (j - p.ncarry);
        d[2 * i] = src[0];
        d[2 * i + 1] = src[1];
    }
}

template <int BPS, typename InT, typename OutT>
hipError_t fsk_go(const FskParams& p, hipStream_t s) {
    using S = FskShape<BPS>;
    const uintptr_t in = reinterpret_cast<uintptr_t>(p.in);
    if (p.n && in % sizeof(InT)) return hipErrorInvalidValue;
    if (p.nsym > 0) {
        const int vw = p.llr ? demap_store_width(p.llr, BPS * DemapOut<OutT>::esz) : 1;
        if (vw < DemapOut<OutT>::esz) return hipErrorInvalidValue;
        const int64_t nblk = (p.nsym + S::NS - 1) / S::NS;
        if (nblk > 0x7fffffff) return hipErrorInvalidValue;
        hipLaunchKernelGGL((fsk_kernel<BPS, InT, OutT>), dim3((unsigned)nblk), dim3(S::NT), 0, s, p,
                           (int)(in % (2 * sizeof(InT)) == 0), vw);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (p.ncarry + p.n - p.nsym * p.sps > 0) {
        hipLaunchKernelGGL((fsk_carry_kernel<InT>), dim3(1), dim3(256), 0, s, p);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <int BPS, typename InT>
hipError_t fsk_out(const FskParams& p, int out_dtype, hipStream_t s) {
    switch (out_dtype) {
    case 0: return fsk_go<BPS, InT, float>(p, s);
    case 1: return fsk_go<BPS, InT, __half>(p, s);
    case 3: return fsk_go<BPS, InT, int8_t>(p, s);
    default: return hipErrorInvalidValue;
    }
}

template <int BPS>
hipError_t fsk_in(const FskParams& p, int in_dtype, int out_dtype, hipStream_t s) {
    switch (in_dtype) {
    case 0: return fsk_out<BPS, float>(p, out_dtype, s);
    case 1: return fsk_out<BPS, __half>(p, out_dtype, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_diff(const DiffParams& p, int in_dtype, int out_dtype, hipStream_t s) {
    if (p.nsym <= 0) return hipSuccess;
    switch (p.bps) {
    case 1: return diff_in<1>(p, in_dtype, out_dtype, s);
    case 2: return diff_in<2>(p, in_dtype, out_dtype, s);
    case 3: return diff_in<3>(p, in_dtype, out_dtype, s);
    case 4: return diff_in<4>(p, in_dtype, out_dtype, s);
    case 5: return diff_in<5>(p, in_dtype, out_dtype, s);
    case 6: return diff_in<6>(p, in_dtype, out_dtype, s);
    case 7: return diff_in<7>(p, in_dtype, out_dtype, s);
    case 8: return diff_in<8>(p, in_dtype, out_dtype, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fsk(const FskParams& p, int in_dtype, int out_dtype, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    switch (p.bps) {
    case 1: return fsk_in<1>(p, in_dtype, out_dtype, s);
    case 2: return fsk_in<2>(p, in_dtype, out_dtype, s);
    case 3: return fsk_in<3>(p, in_dtype, out_dtype, s);
    case 4: return fsk_in<4>(p, in_dtype, out_dtype, s);
    case 5: return fsk_in<5>(p, in_dtype, out_dtype, s);
    case 6: return fsk_in<6>(p, in_dtype, out_dtype, s);
    case 7: return fsk_in<7>(p, in_dtype, out_dtype, s);
    case 8: return fsk_in<8>(p, in_dtype, out_dtype, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mk
