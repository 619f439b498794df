// rust-modem_amd/csrc/modem_demap.hip — soft-decision demapper: per-bit max-log LLRs of the
// matched-filter output (no reference counterpart: the reference ends at hard symbols).
//
//   d(s)            = (re - lut[2s])^2 + (im - lut[2s+1])^2         (differences in f32)
//   llr[k*bps + j]  = scale * (min_{s: bit_j(s)=1} d(s) - min_{s: bit_j(s)=0} d(s)),  j = 0 the MSB
//
// One lane per symbol, a grid-stride loop, the table in LDS (every lane reads the same entry:
// a broadcast). Two paths, chosen at create time:
//   general  any table, bps 1..8: all 2^bps points.
//   axis     the table is a product grid with an even bit split (every QAM at phase 0): the I
//            bits see only the 2^(bps/2) I levels, the Q bits only the Q levels — the common
//            other-axis term cancels in the difference — so 2 * 2^(bps/2) evaluations.
// The minima of a bit are gathered over the binary tree of the symbol index: a node of level L
// (a run of 2^L consecutive indices) hands min(left, right) upwards and feeds `left` to the
// 0-minimum and `right` to the 1-minimum of the bit of weight 2^(L-1). min is exact, so the
// result equals the flat form's (every point into bps of the 2*bps minima) bit for bit, at
// 3 v_min_f32 per point instead of bps. Everything is indexed at compile time: no scratch.
#include "modem_device.h"
#include "modem_llr_store.h"

namespace mk {

namespace {

constexpr int kDemapNT = 256;
constexpr int kDemapMaxBlocks = 2048;   // 8 workgroups per CU; the rest by the grid-stride loop

// Leaf distances: a point of the (i, q) table, or one level of an axis table.
struct LeafPoint {
    const float* tab; float re, im;
    __device__ __forceinline__ float operator()(int s) const {
        const float dx = re - tab[2 * s], dy = im - tab[2 * s + 1];
        return __builtin_fmaf(dy, dy, dx * dx);
    }
};
struct LeafLevel {
    const float* tab; float x;
    __device__ __forceinline__ float operator()(int a) const {
        const float dx = x - tab[a];
        return dx * dx;
    }
};

// min over the indices [base, base + 2^L); the bits of weight < 2^L update their minima
// (bit of weight 2^(L-1) is j = NB - L, MSB first).
template <int L, int NB, typename Leaf>
__device__ __forceinline__ float demap_tree(const Leaf& leaf, int base, float (&m0)[NB], float (&m1)[NB]) {
    if constexpr (L == 0) {
        return leaf(base);
    } else {
        const float a = demap_tree<L - 1, NB>(leaf, base, m0, m1);
        const float b = demap_tree<L - 1, NB>(leaf, base + (1 << (L - 1)), m0, m1);
        m0[NB - L] = __builtin_fminf(m0[NB - L], a);
        m1[NB - L] = __builtin_fminf(m1[NB - L], b);
        return __builtin_fminf(a, b);
    }
}

template <int NB, typename Leaf>
__device__ __forceinline__ void demap_bits(const Leaf& leaf, float scale, float* llr) {
    float m0[NB], m1[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) m0[j] = m1[j] = __builtin_inff();
    (void)demap_tree<NB, NB>(leaf, 0, m0, m1);
#pragma unroll
    for (int j = 0; j < NB; ++j) llr[j] = scale * (m1[j] - m0[j]);
}

// in_f16: f16 I/Q (widened exactly); pair: the (i, q) pairs are naturally aligned (one load);
// vw: bytes per store, the largest power of two <= 16 dividing the lane's B bytes and the
// output base address (wave-uniform).
template <int BPS, bool AXIS, typename OutT>
__global__ __launch_bounds__(kDemapNT) void demap_kernel(const DemapParams p, int in_f16, int pair, int vw) {
    constexpr int H = BPS / 2;
    constexpr int NTAB = AXIS ? 2 * (1 << H) : 2 * (1 << BPS);
    __shared__ __attribute__((aligned(16))) float tab[NTAB];
    for (int i = threadIdx.x; i < NTAB; i += kDemapNT) tab[i] = p.tab[i];
    __syncthreads();

    constexpr int ESZ = DemapOut<OutT>::esz, B = BPS * ESZ, NW = (B + 3) / 4;
    const float scale = p.scale;
    const int64_t stride = (int64_t)gridDim.x * kDemapNT;
    for (int64_t k = (int64_t)blockIdx.x * kDemapNT + threadIdx.x; k < p.nsym; k += stride) {
        float re, im;
        if (in_f16) {
            const __half* x = static_cast<const __half*>(p.iq) + 2 * k;
            if (pair) {
                const __half2 v = *reinterpret_cast<const __half2*>(x);
                re = __low2float(v); im = __high2float(v);
            } else {
                re = __half2float(x[0]); im = __half2float(x[1]);
            }
        } else {
            const float* x = static_cast<const float*>(p.iq) + 2 * k;
            if (pair) {
                const float2 v = *reinterpret_cast<const float2*>(x);
                re = v.x; im = v.y;
            } else {
                re = x[0]; im = x[1];
            }
        }
        float llr[BPS];
        if constexpr (AXIS) {
            demap_bits<H>(LeafLevel{tab, re}, scale, llr);
            demap_bits<H>(LeafLevel{tab + (1 << H), im}, scale, llr + H);
        } else {
            demap_bits<BPS>(LeafPoint{tab, re, im}, scale, llr);
        }
        uint32_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0;
#pragma unroll
        for (int j = 0; j < BPS; ++j) w[j * ESZ / 4] |= DemapOut<OutT>::bits(llr[j]) << (8 * (j * ESZ % 4));
        char* dst = static_cast<char*>(p.llr) + k * B;
        if constexpr (B % 16 == 0) { if (vw == 16) { demap_store<16, B>(dst, w); continue; } }
        if constexpr (B % 8 == 0) { if (vw >= 8) { demap_store<8, B>(dst, w); continue; } }
        if constexpr (B % 4 == 0) { if (vw >= 4) { demap_store<4, B>(dst, w); continue; } }
        if constexpr (B % 2 == 0) { if (vw >= 2) { demap_store<2, B>(dst, w); continue; } }
        if constexpr (ESZ == 1) demap_store<1, B>(dst, w);
    }
}

template <int BPS, bool AXIS, typename OutT>
hipError_t demap_go(const DemapParams& p, int in_f16, hipStream_t s) {
    constexpr int ESZ = DemapOut<OutT>::esz, B = BPS * ESZ;
    const uintptr_t out = reinterpret_cast<uintptr_t>(p.llr), in = reinterpret_cast<uintptr_t>(p.iq);
    const uintptr_t low = (out | (uintptr_t)B | 16u);
    const int vw = (int)(low & (~low + 1));                 // lowest set bit: 1, 2, 4, 8 or 16
    if (vw < ESZ) return hipErrorInvalidValue;              // not even element-aligned
    const int isz = in_f16 ? 2 : 4;
    if (in % isz) return hipErrorInvalidValue;
    const int pair = in % (2 * isz) == 0;
    const int64_t nblk = (p.nsym + kDemapNT - 1) / kDemapNT;
    hipLaunchKernelGGL((demap_kernel<BPS, AXIS, OutT>), dim3((unsigned)(nblk < kDemapMaxBlocks ? nblk : kDemapMaxBlocks)),
                       dim3(kDemapNT), 0, s, p, in_f16, pair, vw);
    return hipGetLastError();
}

template <int BPS, bool AXIS>
hipError_t demap_out(const DemapParams& p, int in_f16, int out_dtype, hipStream_t s) {
    switch (out_dtype) {
    case 0: return demap_go<BPS, AXIS, float>(p, in_f16, s);
    case 1: return demap_go<BPS, AXIS, __half>(p, in_f16, s);
    case 3: return demap_go<BPS, AXIS, int8_t>(p, in_f16, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_demap(const DemapParams& p, bool axis, int in_dtype, int out_dtype, hipStream_t s) {
    if (p.nsym <= 0) return hipSuccess;
    if (in_dtype != 0 && in_dtype != 1) return hipErrorInvalidValue;
    const int f16 = in_dtype == 1;
    if (axis) {
        switch (p.bps) {
        case 2: return demap_out<2, true>(p, f16, out_dtype, s);
        case 4: return demap_out<4, true>(p, f16, out_dtype, s);
        case 6: return demap_out<6, true>(p, f16, out_dtype, s);
        case 8: return demap_out<8, true>(p, f16, out_dtype, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (p.bps) {
    case 1: return demap_out<1, false>(p, f16, out_dtype, s);
    case 2: return demap_out<2, false>(p, f16, out_dtype, s);
    case 3: return demap_out<3, false>(p, f16, out_dtype, s);
    case 4: return demap_out<4, false>(p, f16, out_dtype, s);
    case 5: return demap_out<5, false>(p, f16, out_dtype, s);
    case 6: return demap_out<6, false>(p, f16, out_dtype, s);
    case 7: return demap_out<7, false>(p, f16, out_dtype, s);
    case 8: return demap_out<8, false>(p, f16, out_dtype, s);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace mk
