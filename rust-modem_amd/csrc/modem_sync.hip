// rust-modem_amd/csrc/modem_sync.hip — the feedforward carrier synchronizer on the RX's decimated
// I/Q (no reference counterpart; include/modem_hip.h, "Carrier synchronizer"): block M-th-power
// phase estimates, unwrapped across blocks by an exact integer prefix sum, applied as a
// piecewise-linear derotation. Three launches per call, all over the logical stream
// `carry || in` (the < B symbols the handle kept, then the call's input):
//
// sync_est_kernel: one wave per block, four blocks per workgroup, grid-stride over blocks. Symbol
// i of a block belongs to lane i % 64, row i / 64 (a row is 64 consecutive symbols: one coalesced
// 512-byte read of f32), accumulator (i / 64) % 4. The summation order of P and S is a function of
// i alone:  an accumulator adds its rows ascending from 0 (at most 16 of them at B = 4096);
// lane = (acc0 + acc1) + (acc2 + acc3); then the 6-level butterfly over lane distances
// 32, 16, 8, 4, 2, 1 (a + b is commutative: every lane ends with the same bits). Lane 0 forms
// the angle and the quality and writes Phi[b], q[b].
//
// sync_scan_kernel: one workgroup. theta[b] = theta[b-1] + (sext(Phi[b] - Phi[b-1]) >> lm) is a
// prefix sum of local terms in the ring of 64-bit integers, so its grouping is free: 4 blocks per
// lane, a shuffle scan over the wave, LDS across the four waves, 1024 blocks per round. Reads the
// handle's {theta, Phi, d} slot and writes the other one.
//
// sync_apply_kernel: the channel kernel's shape. A lane takes groups of 4 consecutive symbols
// (never across a block edge: B is a multiple of 64) in a grid-stride loop, with 16-byte loads
// and stores where the group is 16-byte aligned and lies in the input, symbol by symbol (or
// component by component) otherwise; the phase of a group's first symbol costs one 64-bit
// multiply, the next three an add each. The same launch moves the leftover symbols into the
// handle's other carry slot.
//
// Plain vector stores only, no atomics, everything indexed at compile time: no scratch.
#include "modem_device.h"
#include "modem_sync_math.h"

namespace mk {

namespace {

constexpr int kSyncNT = 256;
constexpr int kSyncMaxBlocks = 2048;    // 8 workgroups per CU; the rest by the grid-stride loops
constexpr int kSyncG = 4;               // symbols per lane and step of the apply kernel
constexpr int kSyncAcc = 4;             // accumulators per lane of the estimator
constexpr int kScanPer = 4;             // blocks per lane and round of the scan

typedef uint32_t sv4u __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ T sld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)p;
}
template <typename T> __device__ __forceinline__ void sst(void* p, T v) { *(__attribute__((address_space(1))) T*)p = v; }

__device__ __forceinline__ void sync_unpack_h2(uint32_t w, float& a, float& b) {
    const __half2 h = *reinterpret_cast<const __half2*>(&w);
    a = __low2float(h);
    b = __high2float(h);
}
__device__ __forceinline__ uint32_t sync_pack_h2(float a, float b) {     // round to nearest even, as the TX stores
    const __half2 h = __floats2half2_rn(a, b);
    return *reinterpret_cast<const uint32_t*>(&h);
}

// Symbol I/O of one dtype, the accesses of modem_chan.hip's ChanIO: load4 / store4 = the 16-byte
// accesses of 4 symbols (base + s symbols 16-byte aligned), load1 / store1 = one symbol (pair:
// symbol-aligned, else two component accesses).
template <typename T> struct SyncIO;
template <> struct SyncIO<float> {
    static constexpr int ssz = 8;
    __device__ static void load4(const void* base, int64_t s, float (&v)[2 * kSyncG]) {
        const char* p = static_cast<const char*>(base) + s * ssz;
        const gv4f a = sld<gv4f>(p), b = sld<gv4f>(p + 16);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ static void store4(void* base, int64_t s, const float (&v)[2 * kSyncG]) {
        char* p = static_cast<char*>(base) + s * ssz;
        sst<gv4f>(p, (gv4f){v[0], v[1], v[2], v[3]});
        sst<gv4f>(p + 16, (gv4f){v[4], v[5], v[6], v[7]});
    }
    __device__ static void load1(const void* base, int64_t s, bool pair, float& re, float& im) {
        const char* p = static_cast<const char*>(base) + s * ssz;
        if (pair) {
            const gv2f a = sld<gv2f>(p);
            re = a.x; im = a.y;
        } else {
            re = sld<float>(p); im = sld<float>(p + 4);
        }
    }
    __device__ static void store1(void* base, int64_t s, bool pair, float re, float im) {
        char* p = static_cast<char*>(base) + s * ssz;
        if (pair) {
            sst<gv2f>(p, (gv2f){re, im});
        } else {
            sst<float>(p, re); sst<float>(p + 4, im);
        }
    }
};
template <> struct SyncIO<__half> {
    static constexpr int ssz = 4;
    __device__ static void load4(const void* base, int64_t s, float (&v)[2 * kSyncG]) {
        const sv4u a = sld<sv4u>(static_cast<const char*>(base) + s * ssz);
        sync_unpack_h2(a.x, v[0], v[1]); sync_unpack_h2(a.y, v[2], v[3]);
        sync_unpack_h2(a.z, v[4], v[5]); sync_unpack_h2(a.w, v[6], v[7]);
    }
    __device__ static void store4(void* base, int64_t s, const float (&v)[2 * kSyncG]) {
        sst<sv4u>(static_cast<char*>(base) + s * ssz,
                  (sv4u){sync_pack_h2(v[0], v[1]), sync_pack_h2(v[2], v[3]), sync_pack_h2(v[4], v[5]),
                         sync_pack_h2(v[6], v[7])});
    }
    __device__ static void load1(const void* base, int64_t s, bool pair, float& re, float& im) {
        const char* p = static_cast<const char*>(base) + s * ssz;
        if (pair) {
            sync_unpack_h2(sld<uint32_t>(p), re, im);
        } else {
            sync_unpack_h2((uint32_t)sld<uint16_t>(p) | (uint32_t)sld<uint16_t>(p + 2) << 16, re, im);
        }
    }
    __device__ static void store1(void* base, int64_t s, bool pair, float re, float im) {
        char* p = static_cast<char*>(base) + s * ssz;
        const uint32_t w = sync_pack_h2(re, im);
        if (pair) {
            sst<uint32_t>(p, w);
        } else {
            sst<uint16_t>(p, (uint16_t)w); sst<uint16_t>(p + 2, (uint16_t)(w >> 16));
        }
    }
};

// symbol j of the logical stream carry || in (j < ncarry + n)
template <typename InT>
__device__ __forceinline__ void sync_load(const SyncParams& p, int64_t j, bool pair, float& re, float& im) {
    if (j < p.ncarry) SyncIO<InT>::load1(p.carry, j, true, re, im);
    else SyncIO<InT>::load1(p.in, j - p.ncarry, pair, re, im);
}

template <int LM, typename InT>
__global__ __launch_bounds__(kSyncNT) void sync_est_kernel(const SyncParams p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t B = (int64_t)1 << p.lb;
    const int rows = (int)(B >> 6);
    const bool pair = p.in_align >= 1;
    constexpr int W = kSyncNT / 64;
    for (int64_t b = (int64_t)blockIdx.x * W + wave; b < p.nblk; b += (int64_t)gridDim.x * W) {
        float ar[kSyncAcc], ai[kSyncAcc], as[kSyncAcc];
#pragma unroll
        for (int a = 0; a < kSyncAcc; ++a) ar[a] = ai[a] = as[a] = 0.f;
        const int64_t j0 = b * B + lane;
        for (int r0 = 0; r0 < rows; r0 += kSyncAcc) {
#pragma unroll
            for (int a = 0; a < kSyncAcc; ++a) {
                if (r0 + a < rows) {
                    float re, im, zr, zi, mg;
                    sync_load<InT>(p, j0 + 64 * (int64_t)(r0 + a), pair, re, im);
                    sync_power(re, im, p.nrm, LM, zr, zi, mg);
                    ar[a] = ar[a] + zr;
                    ai[a] = ai[a] + zi;
                    as[a] = as[a] + mg;
                }
            }
        }
        float pr = (ar[0] + ar[1]) + (ar[2] + ar[3]);
        float pi = (ai[0] + ai[1]) + (ai[2] + ai[3]);
        float ss = (as[0] + as[1]) + (as[2] + as[3]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            pr = pr + __shfl_xor(pr, o, 64);
            pi = pi + __shfl_xor(pi, o, 64);
            ss = ss + __shfl_xor(ss, o, 64);
        }
        if (lane == 0) {
            p.phi[b] = ((uint64_t)sync_atan2_turn(pi, pr) << 32) - p.ref;
            p.q[b] = sync_quality(pr, pi, ss);
        }
    }
}

__global__ __launch_bounds__(kSyncNT) void sync_scan_kernel(const SyncParams p) {
    __shared__ uint64_t wsum[kSyncNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t last = p.nblk - 1;
    uint64_t base = p.state[0];
    if (tid == 0) p.th[0] = base;
    for (int64_t c0 = 0; c0 < p.nblk; c0 += kScanPer * kSyncNT) {
        const int64_t b0 = c0 + kScanPer * tid;
        uint64_t inc[kScanPer], run = 0;
        uint64_t prev = b0 == 0 ? p.state[1] : (b0 <= last ? p.phi[b0 - 1] : 0);
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            if (b0 + j <= last) {
                const uint64_t phi = p.phi[b0 + j];
                run += (uint64_t)((int64_t)(phi - prev) >> p.lm);
                prev = phi;
            }
            inc[j] = run;
        }
        uint64_t incl = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t v = __shfl_up((unsigned long long)incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint64_t off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < kSyncNT / 64; ++w) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        off += incl - run;                                   // theta of the block before b0
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            if (b0 + j <= last) {
                const uint64_t theta = off + inc[j];
                p.th[1 + b0 + j] = theta;
                if (b0 + j == last) {
                    const uint64_t before = off + (j ? inc[j ? j - 1 : 0] : 0);
                    p.state_new[0] = theta;
                    p.state_new[1] = prev;                   // Phi of the last block
                    p.state_new[2] = (p.first && last == 0) ? 0 : theta - before;
                }
            }
        }
        base += tot;
        __syncthreads();                                     // wsum is rewritten in the next round
    }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(kSyncNT) void sync_apply_kernel(const SyncParams p) {
    const int64_t B = (int64_t)1 << p.lb, nout = p.nblk << p.lb, ngroups = nout / kSyncG;
    const int64_t stride = (int64_t)gridDim.x * kSyncNT, gid = (int64_t)blockIdx.x * kSyncNT + threadIdx.x;
    const bool in_wide = p.in_align == 2, in_pair = p.in_align >= 1;
    const bool out_wide = p.out_align == 2, out_pair = p.out_align >= 1;
    for (int64_t g = gid; g < ngroups; g += stride) {
        const int64_t j = kSyncG * g, b = j >> p.lb, i0 = j & (B - 1);
        const uint64_t theta = p.th[b + 1];
        int64_t d = (int64_t)(theta - p.th[b]);
        if (p.first && b == 0) d = 0;
        const int64_t s = p.flat ? 0 : d >> (p.lb + 1);
        float v[2 * kSyncG];
        if (in_wide && j >= p.ncarry) {
            SyncIO<InT>::load4(p.in, j - p.ncarry, v);
        } else {
#pragma unroll
            for (int k = 0; k < kSyncG; ++k) sync_load<InT>(p, j + k, in_pair, v[2 * k], v[2 * k + 1]);
        }
        const uint64_t ph = sync_line(theta, s, i0, B), dph = (uint64_t)(2 * s);
#pragma unroll
        for (int k = 0; k < kSyncG; ++k) sync_derotate(v[2 * k], v[2 * k + 1], ph + (uint64_t)k * dph);
        if (out_wide) {
            SyncIO<OutT>::store4(p.out, j, v);
        } else {
#pragma unroll
            for (int k = 0; k < kSyncG; ++k) SyncIO<OutT>::store1(p.out, j + k, out_pair, v[2 * k], v[2 * k + 1]);
        }
    }
    // the symbols after the last whole block: into the other carry slot, as values of the input dtype
    const int64_t left = (int64_t)p.ncarry + p.n - nout;
    for (int64_t t = gid; t < left; t += stride) {
        float re, im;
        sync_load<InT>(p, nout + t, in_pair, re, im);
        SyncIO<InT>::store1(p.carry_new, t, true, re, im);
    }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(kSyncNT) void sync_flush_kernel(const SyncParams p) {
    const int64_t B = (int64_t)1 << p.lb;
    const uint64_t theta = p.state[0];
    const int64_t s = p.flat ? 0 : (int64_t)p.state[2] >> (p.lb + 1);
    const bool out_pair = p.out_align >= 1;
    for (int64_t t = (int64_t)blockIdx.x * kSyncNT + threadIdx.x; t < p.ncarry; t += (int64_t)gridDim.x * kSyncNT) {
        float re, im;
        SyncIO<InT>::load1(p.carry, t, true, re, im);
        sync_derotate(re, im, sync_line(theta, s, t + B, B));
        SyncIO<OutT>::store1(p.out, t, out_pair, re, im);
    }
}

unsigned sync_grid(int64_t items, int per_block) {
    const int64_t nblk = (items + per_block - 1) / per_block;
    return (unsigned)(nblk < 1 ? 1 : nblk < kSyncMaxBlocks ? nblk : kSyncMaxBlocks);
}

template <typename InT>
hipError_t sync_est_go(const SyncParams& p, hipStream_t s) {
    const dim3 grid(sync_grid(p.nblk, kSyncNT / 64)), block(kSyncNT);
    switch (p.lm) {
    case 1: hipLaunchKernelGGL((sync_est_kernel<1, InT>), grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL((sync_est_kernel<2, InT>), grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL((sync_est_kernel<3, InT>), grid, block, 0, s, p); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename InT, typename OutT>
hipError_t sync_go(const SyncParams& p, hipStream_t s) {
    hipError_t e;
    if (p.nblk > 0) {
        if ((e = sync_est_go<InT>(p, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(sync_scan_kernel, dim3(1), dim3(kSyncNT), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int64_t ngroups = (p.nblk << p.lb) / kSyncG, left = (int64_t)p.ncarry + p.n - (p.nblk << p.lb);
    hipLaunchKernelGGL((sync_apply_kernel<InT, OutT>), dim3(sync_grid(ngroups > left ? ngroups : left, kSyncNT)),
                       dim3(kSyncNT), 0, s, p);
    return hipGetLastError();
}

template <typename InT, typename OutT>
hipError_t sync_flush_go(const SyncParams& p, hipStream_t s) {
    hipLaunchKernelGGL((sync_flush_kernel<InT, OutT>), dim3(sync_grid(p.ncarry, kSyncNT)), dim3(kSyncNT), 0, s, p);
    return hipGetLastError();
}

// 2: groups of 4 symbols counted from `first_group` are 16-byte aligned; 1: symbols are; 0: elements; -1: not even those
int sync_align(const void* base, uintptr_t first_group, int ssz) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(base);
    if (a % (ssz / 2)) return -1;
    return first_group % 16 == 0 ? 2 : a % ssz == 0 ? 1 : 0;
}

bool sync_set_align(SyncParams& p, int in_dtype, int out_dtype) {
    if ((in_dtype != 0 && in_dtype != 1) || (out_dtype != 0 && out_dtype != 1)) return false;
    const int isz = in_dtype ? 4 : 8, osz = out_dtype ? 4 : 8;
    // group g of the logical stream starts ncarry symbols before in + 4 g symbols
    p.in_align = p.in ? sync_align(p.in, reinterpret_cast<uintptr_t>(p.in) - (uintptr_t)p.ncarry * isz, isz) : 2;
    p.out_align = p.out ? sync_align(p.out, reinterpret_cast<uintptr_t>(p.out), osz) : 2;
    return p.in_align >= 0 && p.out_align >= 0;
}

}  // namespace

hipError_t launch_sync(const SyncParams& p0, int in_dtype, int out_dtype, hipStream_t s) {
    SyncParams p = p0;
    if (!sync_set_align(p, in_dtype, out_dtype) || p.lb < 6 || p.lb > 12 || p.ncarry < 0 || p.ncarry >= (1 << p.lb) ||
        p.n < 0 || p.nblk != ((int64_t)p.ncarry + p.n) >> p.lb) return hipErrorInvalidValue;
    switch (in_dtype * 2 + out_dtype) {
    case 0: return sync_go<float, float>(p, s);
    case 1: return sync_go<float, __half>(p, s);
    case 2: return sync_go<__half, float>(p, s);
    default: return sync_go<__half, __half>(p, s);
    }
}

hipError_t launch_sync_flush(const SyncParams& p0, int in_dtype, int out_dtype, hipStream_t s) {
    SyncParams p = p0;
    if (p.ncarry <= 0) return hipSuccess;
    if (!sync_set_align(p, in_dtype, out_dtype) || p.lb < 6 || p.lb > 12 || p.ncarry >= (1 << p.lb)) return hipErrorInvalidValue;
    switch (in_dtype * 2 + out_dtype) {
    case 0: return sync_flush_go<float, float>(p, s);
    case 1: return sync_flush_go<float, __half>(p, s);
    case 2: return sync_flush_go<__half, float>(p, s);
    default: return sync_flush_go<__half, __half>(p, s);
    }
}

}  // namespace mk
