// rust-modem_amd/csrc/modem_timing.hip — the feedforward symbol timing synchronizer on the RX's
// matched-filter output at sample rate (no reference counterpart; include/modem_hip.h, "Symbol
// timing synchronizer"): block square-law (Oerder & Meyr) delay estimates, unwrapped across blocks
// by an exact integer prefix sum, applied as a piecewise-linear delay through a 4-tap cubic Lagrange
// interpolator. Three launches per call, all over the logical stream `pre || in` (the H = 2 span N
// + 1 samples of history and the samples of the incomplete block the handle kept, then the call's
// input):
//
// timing_est_kernel: one wave per block, four blocks per workgroup, grid-stride over blocks. The
// sample at offset u of a block belongs to pair t = u / 2, lane t % 64, row t / 64 (a row is 128
// consecutive samples: one coalesced 1024-byte read of f32), accumulator (t / 64) % 4, component
// u % 2. The summation order of the E_p is a function of u alone: an accumulator adds its rows
// ascending from 0 (at most 64 of them at B = 4096, N = 8); lane = (acc0 + acc1) + (acc2 + acc3);
// then the butterfly over lane distances 32, 16, 8, 4 (and 2 for N = 4), which joins the lanes of
// one sample phase p = u % N. Lane 0 gathers the N sums, forms the line, the angle and the quality
// and writes Phi[b], q[b].
//
// timing_scan_kernel: one workgroup. D[b] = D[b-1] + sext32(Phi[b] - Phi[b-1]) is a prefix sum of
// local terms in the 64-bit integers, so its grouping is free: 4 blocks per lane, a shuffle scan
// over the wave, LDS across the four waves, 1024 blocks per round. Reads the handle's {D, Phi, d}
// slot and writes the other one.
//
// timing_apply_kernel: a lane takes groups of 4 consecutive output symbols (never across a block
// edge: B is a multiple of 32) in a grid-stride loop; each symbol gathers its 4 neighbouring
// samples with 8-byte loads (4-byte for f16) where samples are aligned and lie in the input,
// component by component otherwise, and the group is stored with 16-byte stores where aligned.
// The taps of a wave's 256 symbols cover one contiguous run of 256 N samples, so the gather is
// served by the vector cache and L2: a sample comes from HBM once. The same launch moves the last
// H + left samples of the logical stream into the handle's other slot.
//
// Plain vector stores only, no atomics, everything indexed at compile time: no scratch.
#include "modem_device.h"
#include "modem_timing_math.h"

namespace mk {

namespace {

constexpr int kTimNT = 256;
constexpr int kTimMaxBlocks = 2048;     // 8 workgroups per CU; the rest by the grid-stride loops
constexpr int kTimG = 4;                // output symbols per lane and step of the apply kernel
constexpr int kTimAcc = 4;              // accumulators per lane of the estimator
constexpr int kTimScanPer = 4;          // blocks per lane and round of the scan

typedef uint32_t tv4u __attribute__((ext_vector_type(4)));
typedef uint32_t tv2u __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ T tld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)p;
}
template <typename T> __device__ __forceinline__ void tst(void* p, T v) { *(__attribute__((address_space(1))) T*)p = v; }

__device__ __forceinline__ void tim_unpack_h2(uint32_t w, float& a, float& b) {
    const __half2 h = *reinterpret_cast<const __half2*>(&w);
    a = __low2float(h);
    b = __high2float(h);
}
__device__ __forceinline__ uint32_t tim_pack_h2(float a, float b) {      // round to nearest even
    const __half2 h = __floats2half2_rn(a, b);
    return *reinterpret_cast<const uint32_t*>(&h);
}

// Sample I/O of one dtype: load2 = the wide access of 2 samples (16 bytes of f32, 8 of f16; base +
// s samples aligned to it), load1 / store1 = one sample (pair: sample-aligned, else two component
// accesses), store4 = the 16-byte stores of 4 samples, move1 = a sample's bits.
template <typename T> struct TimIO;
template <> struct TimIO<float> {
    static constexpr int ssz = 8;
    __device__ static void load2(const void* base, int64_t s, float (&v)[4]) {
        const gv4f a = tld<gv4f>(static_cast<const char*>(base) + s * ssz);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
    __device__ static void load1(const void* base, int64_t s, bool pair, float& re, float& im) {
        const char* p = static_cast<const char*>(base) + s * ssz;
        if (pair) {
            const gv2f a = tld<gv2f>(p);
            re = a.x; im = a.y;
        } else {
            re = tld<float>(p); im = tld<float>(p + 4);
        }
    }
    __device__ static void store4(void* base, int64_t s, const float (&v)[2 * kTimG]) {
        char* p = static_cast<char*>(base) + s * ssz;
        tst<gv4f>(p, (gv4f){v[0], v[1], v[2], v[3]});
        tst<gv4f>(p + 16, (gv4f){v[4], v[5], v[6], v[7]});
    }
    __device__ static void store1(void* base, int64_t s, bool pair, float re, float im) {
        char* p = static_cast<char*>(base) + s * ssz;
        if (pair) {
            tst<gv2f>(p, (gv2f){re, im});
        } else {
            tst<float>(p, re); tst<float>(p + 4, im);
        }
    }
};
template <> struct TimIO<__half> {
    static constexpr int ssz = 4;
    __device__ static void load2(const void* base, int64_t s, float (&v)[4]) {
        const tv2u a = tld<tv2u>(static_cast<const char*>(base) + s * ssz);
        tim_unpack_h2(a.x, v[0], v[1]); tim_unpack_h2(a.y, v[2], v[3]);
    }
    __device__ static void load1(const void* base, int64_t s, bool pair, float& re, float& im) {
        const char* p = static_cast<const char*>(base) + s * ssz;
        if (pair) {
            tim_unpack_h2(tld<uint32_t>(p), re, im);
        } else {
            tim_unpack_h2((uint32_t)tld<uint16_t>(p) | (uint32_t)tld<uint16_t>(p + 2) << 16, re, im);
        }
    }
    __device__ static void store4(void* base, int64_t s, const float (&v)[2 * kTimG]) {
        tst<tv4u>(static_cast<char*>(base) + s * ssz,
                  (tv4u){tim_pack_h2(v[0], v[1]), tim_pack_h2(v[2], v[3]), tim_pack_h2(v[4], v[5]),
                         tim_pack_h2(v[6], v[7])});
    }
    __device__ static void store1(void* base, int64_t s, bool pair, float re, float im) {
        char* p = static_cast<char*>(base) + s * ssz;
        const uint32_t w = tim_pack_h2(re, im);
        if (pair) {
            tst<uint32_t>(p, w);
        } else {
            tst<uint16_t>(p, (uint16_t)w); tst<uint16_t>(p + 2, (uint16_t)(w >> 16));
        }
    }
};

// sample j of the logical stream pre || in (0 <= j < npre + n)
template <typename InT>
__device__ __forceinline__ void tim_load(const TimingParams& p, int64_t j, bool pair, float& re, float& im) {
    if (j < p.npre) TimIO<InT>::load1(p.pre, j, true, re, im);
    else TimIO<InT>::load1(p.in, j - p.npre, pair, re, im);
}

__device__ __forceinline__ float tim_energy(float re, float im) {
#pragma clang fp contract(off)
    return __builtin_fmaf(re, re, im * im);
}

template <int LN, typename InT>
__global__ __launch_bounds__(kTimNT) void timing_est_kernel(const TimingParams p) {
#pragma clang fp contract(off)
    constexpr int N = 1 << LN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t BN = (int64_t)1 << (p.lb + LN);
    const int rows = (int)(BN >> 7);
    const int64_t H = 2 * (int64_t)p.span * N + 1;
    const bool pair = p.in_align >= 1, wide = p.in_align == 2;
    constexpr int W = kTimNT / 64;
    for (int64_t b = (int64_t)blockIdx.x * W + wave; b < p.nblk; b += (int64_t)gridDim.x * W) {
        float a0[kTimAcc], a1[kTimAcc];
#pragma unroll
        for (int a = 0; a < kTimAcc; ++a) a0[a] = a1[a] = 0.f;
        const int64_t j0 = H + b * BN + 2 * lane;
        for (int r0 = 0; r0 < rows; r0 += kTimAcc) {
#pragma unroll
            for (int a = 0; a < kTimAcc; ++a) {
                if (r0 + a < rows) {
                    const int64_t j = j0 + 128 * (int64_t)(r0 + a);
                    float v[4];
                    if (wide && j >= p.npre) {
                        TimIO<InT>::load2(p.in, j - p.npre, v);
                    } else {
                        tim_load<InT>(p, j, pair, v[0], v[1]);
                        tim_load<InT>(p, j + 1, pair, v[2], v[3]);
                    }
                    a0[a] = a0[a] + tim_energy(v[0], v[1]);
                    a1[a] = a1[a] + tim_energy(v[2], v[3]);
                }
            }
        }
        float e0 = (a0[0] + a0[1]) + (a0[2] + a0[3]);
        float e1 = (a1[0] + a1[1]) + (a1[2] + a1[3]);
#pragma unroll
        for (int o = 32; o >= N / 2; o >>= 1) {
            e0 = e0 + __shfl_xor(e0, o, 64);
            e1 = e1 + __shfl_xor(e1, o, 64);
        }
        float E[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) E[k] = 0.f;
#pragma unroll
        for (int k = 0; k < N; ++k) E[k] = __shfl((k & 1) ? e1 : e0, k >> 1, 64);
        if (lane == 0) {
            float re, im, S;
            timing_line(E, LN, re, im, S);
            p.phi[b] = timing_phi(re, im);
            p.q[b] = sync_quality(re, im, S);
        }
    }
}

__global__ __launch_bounds__(kTimNT) void timing_scan_kernel(const TimingParams p) {
    __shared__ int64_t wsum[kTimNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t last = p.nblk - 1;
    int64_t base = p.state[0];
    if (tid == 0) p.th[0] = base;
    for (int64_t c0 = 0; c0 < p.nblk; c0 += kTimScanPer * kTimNT) {
        const int64_t b0 = c0 + kTimScanPer * tid;
        int64_t inc[kTimScanPer], run = 0;
        uint32_t prev = b0 == 0 ? (uint32_t)p.state[1] : (b0 <= last ? p.phi[b0 - 1] : 0u);
#pragma unroll
        for (int j = 0; j < kTimScanPer; ++j) {
            if (b0 + j <= last) {
                const uint32_t phi = p.phi[b0 + j];
                run += (int64_t)(int32_t)(phi - prev);
                prev = phi;
            }
            inc[j] = run;
        }
        int64_t incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t v = (int64_t)__shfl_up((unsigned long long)incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int64_t off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < kTimNT / 64; ++w) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        off += incl - run;                                   // D of the block before b0
#pragma unroll
        for (int j = 0; j < kTimScanPer; ++j) {
            if (b0 + j <= last) {
                const int64_t D = off + inc[j];
                p.th[1 + b0 + j] = D;
                if (b0 + j == last) {
                    const int64_t before = off + (j ? inc[j ? j - 1 : 0] : 0);
                    p.state_new[0] = D;
                    p.state_new[1] = (int64_t)prev;          // Phi of the last block
                    p.state_new[2] = (p.first && last == 0) ? 0 : D - before;
                }
            }
        }
        base += tot;
        __syncthreads();                                     // wsum is rewritten in the next round
    }
}

// One output symbol: the 4 samples from index jb of the logical stream (jb + 3 < lim; samples at
// or past lim read as zero: the flush), weighted by the coefficients of mu.
template <typename InT>
__device__ __forceinline__ void tim_interp(const TimingParams& p, int64_t jb, int64_t lim, bool pair, float mu,
                                           float& re, float& im) {
    float xr[4], xi[4];
    if (pair && jb >= p.npre && jb + 3 < lim) {
#pragma unroll
        for (int t = 0; t < 4; ++t) TimIO<InT>::load1(p.in, jb - p.npre + t, true, xr[t], xi[t]);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            xr[t] = xi[t] = 0.f;
            if (jb + t < lim) tim_load<InT>(p, jb + t, pair, xr[t], xi[t]);
        }
    }
    float c[4];
    timing_coefs(mu, c);
    re = timing_dot(c, xr[0], xr[1], xr[2], xr[3]);
    im = timing_dot(c, xi[0], xi[1], xi[2], xi[3]);
}

template <int LN, typename InT, typename OutT>
__global__ __launch_bounds__(kTimNT) void timing_apply_kernel(const TimingParams p) {
    constexpr int N = 1 << LN;
    const int64_t B = (int64_t)1 << p.lb, nout = p.nblk << p.lb, ngroups = nout / kTimG;
    const int64_t stride = (int64_t)gridDim.x * kTimNT, gid = (int64_t)blockIdx.x * kTimNT + threadIdx.x;
    const int64_t H = 2 * (int64_t)p.span * N + 1, total = (int64_t)p.npre + p.n;
    const bool in_pair = p.in_align >= 1, out_wide = p.out_align == 2, out_pair = p.out_align >= 1;
    for (int64_t g = gid; g < ngroups; g += stride) {
        const int64_t k0 = kTimG * g, b = k0 >> p.lb, i0 = k0 & (B - 1);
        const int64_t D = p.th[b + 1];
        int64_t d = D - p.th[b];
        if (p.first && b == 0) d = 0;
        const int64_t s = p.flat ? 0 : d >> (p.lb + 1);
        const int64_t blk = H + ((b << p.lb) << LN);                  // the block's first sample
        float v[2 * kTimG];
#pragma unroll
        for (int k = 0; k < kTimG; ++k) {
            const int64_t Q = timing_pos(D, s, i0 + k, i0 + k, p.lb, LN, p.span);
            tim_interp<InT>(p, blk + (Q >> 32) - 1, total, in_pair, timing_mu(Q), v[2 * k], v[2 * k + 1]);
        }
        if (out_wide) {
            TimIO<OutT>::store4(p.out, k0, v);
        } else {
#pragma unroll
            for (int k = 0; k < kTimG; ++k) TimIO<OutT>::store1(p.out, k0 + k, out_pair, v[2 * k], v[2 * k + 1]);
        }
    }
    // the history of the next block and the samples after the last whole block: into the other
    // slot, as values of the input dtype
    const int64_t src = (p.nblk << p.lb) << LN, keep = total - src;
    for (int64_t t = gid; t < keep; t += stride) {
        float re, im;
        tim_load<InT>(p, src + t, in_pair, re, im);
        TimIO<InT>::store1(p.pre_new, t, true, re, im);
    }
}

template <int LN, typename InT, typename OutT>
__global__ __launch_bounds__(kTimNT) void timing_flush_kernel(const TimingParams p) {
    constexpr int N = 1 << LN;
    const int64_t B = (int64_t)1 << p.lb, H = 2 * (int64_t)p.span * N + 1;
    const int64_t stride = (int64_t)gridDim.x * kTimNT, gid = (int64_t)blockIdx.x * kTimNT + threadIdx.x;
    const int64_t D = p.state[0];
    const int64_t s = p.flat ? 0 : p.state[2] >> (p.lb + 1);
    const bool out_pair = p.out_align >= 1;
    for (int64_t i = gid; i < p.nflush; i += stride) {
        const int64_t Q = timing_pos(D, s, i + B, i, p.lb, LN, p.span);
        float re, im;
        tim_interp<InT>(p, H + (Q >> 32) - 1, p.npre, true, timing_mu(Q), re, im);
        TimIO<OutT>::store1(p.out, i, out_pair, re, im);
    }
    for (int64_t t = gid; t < H; t += stride) TimIO<InT>::store1(p.pre_new, t, true, 0.f, 0.f);
}

unsigned tim_grid(int64_t items, int per_block) {
    const int64_t nblk = (items + per_block - 1) / per_block;
    return (unsigned)(nblk < 1 ? 1 : nblk < kTimMaxBlocks ? nblk : kTimMaxBlocks);
}

template <int LN, typename InT, typename OutT>
hipError_t tim_go(const TimingParams& p, hipStream_t s) {
    hipError_t e;
    if (p.nblk > 0) {
        hipLaunchKernelGGL((timing_est_kernel<LN, InT>), dim3(tim_grid(p.nblk, kTimNT / 64)), dim3(kTimNT), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(timing_scan_kernel, dim3(1), dim3(kTimNT), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int64_t ngroups = (p.nblk << p.lb) / kTimG, keep = (int64_t)p.npre + p.n - ((p.nblk << p.lb) << LN);
    hipLaunchKernelGGL((timing_apply_kernel<LN, InT, OutT>), dim3(tim_grid(ngroups > keep ? ngroups : keep, kTimNT)),
                       dim3(kTimNT), 0, s, p);
    return hipGetLastError();
}

template <int LN, typename InT, typename OutT>
hipError_t tim_flush_go(const TimingParams& p, hipStream_t s) {
    const int64_t H = 2 * (int64_t)p.span * (1 << LN) + 1;
    hipLaunchKernelGGL((timing_flush_kernel<LN, InT, OutT>), dim3(tim_grid(p.nflush > H ? p.nflush : H, kTimNT)),
                       dim3(kTimNT), 0, s, p);
    return hipGetLastError();
}

template <int LN>
hipError_t tim_dispatch(const TimingParams& p, bool flush, int in_dtype, int out_dtype, hipStream_t s) {
    switch (in_dtype * 2 + out_dtype) {
    case 0: return flush ? tim_flush_go<LN, float, float>(p, s) : tim_go<LN, float, float>(p, s);
    case 1: return flush ? tim_flush_go<LN, float, __half>(p, s) : tim_go<LN, float, __half>(p, s);
    case 2: return flush ? tim_flush_go<LN, __half, float>(p, s) : tim_go<LN, __half, float>(p, s);
    default: return flush ? tim_flush_go<LN, __half, __half>(p, s) : tim_go<LN, __half, __half>(p, s);
    }
}

// The common checks, and the alignments: in 2 = the pairs of samples counted from a block's first
// sample are aligned to their wide access, out 2 = groups of 4 symbols are 16-byte aligned;
// 1 = samples are aligned; 0 = elements are.
bool tim_prepare(TimingParams& p, int in_dtype, int out_dtype) {
    if ((in_dtype != 0 && in_dtype != 1) || (out_dtype != 0 && out_dtype != 1)) return false;
    if (p.lb < 5 || p.lb > 12 || (p.ln != 2 && p.ln != 3) || p.span < 1 || p.span > 16) return false;
    const int64_t H = 2 * (int64_t)p.span * (1 << p.ln) + 1, BN = (int64_t)1 << (p.lb + p.ln);
    if (p.npre < H || p.npre >= H + BN) return false;
    const uintptr_t isz = in_dtype ? 4 : 8, osz = out_dtype ? 4 : 8;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(p.in), oa = reinterpret_cast<uintptr_t>(p.out);
    if (ia % (isz / 2) || oa % (osz / 2)) return false;
    // pair t of block b starts (b B N + 2 t - carried) samples into `in`
    p.in_align = !p.in ? 2 : (ia - (uintptr_t)(p.npre - H) * isz) % (2 * isz) == 0 ? 2 : ia % isz == 0 ? 1 : 0;
    p.out_align = !p.out ? 2 : oa % 16 == 0 ? 2 : oa % osz == 0 ? 1 : 0;
    return true;
}

}  // namespace

hipError_t launch_timing(const TimingParams& p0, int in_dtype, int out_dtype, hipStream_t s) {
    TimingParams p = p0;
    if (!tim_prepare(p, in_dtype, out_dtype) || p.n < 0) return hipErrorInvalidValue;
    const int64_t H = 2 * (int64_t)p.span * (1 << p.ln) + 1;
    if (p.nblk != ((int64_t)p.npre - H + p.n) >> (p.lb + p.ln)) return hipErrorInvalidValue;
    return p.ln == 2 ? tim_dispatch<2>(p, false, in_dtype, out_dtype, s) : tim_dispatch<3>(p, false, in_dtype, out_dtype, s);
}

hipError_t launch_timing_flush(const TimingParams& p0, int in_dtype, int out_dtype, hipStream_t s) {
    TimingParams p = p0;
    p.in = nullptr;
    p.n = 0;
    if (!tim_prepare(p, in_dtype, out_dtype)) return hipErrorInvalidValue;
    const int64_t H = 2 * (int64_t)p.span * (1 << p.ln) + 1;
    if (p.nflush < 0 || p.nflush != (p.npre - H) >> p.ln) return hipErrorInvalidValue;
    return p.ln == 2 ? tim_dispatch<2>(p, true, in_dtype, out_dtype, s) : tim_dispatch<3>(p, true, in_dtype, out_dtype, s);
}

}  // namespace mk
