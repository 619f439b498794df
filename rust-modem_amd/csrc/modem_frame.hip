// rust-modem_amd/csrc/modem_frame.hip — the data-aided frame synchronizer on the carrier
// synchronizer's output (no reference counterpart; include/modem_hip.h, "Frame synchronizer"): a
// unique word is correlated against the symbol stream, peaks of the normalised correlation are
// picked, and the hits (position, angle, metric) are stored in ascending order; a stateless gather
// cuts the frames out and takes the M-fold rotation off. Three launches per call, all over the
// logical stream `carry || in` (the <= 2W + L - 1 symbols the handle kept, then the call's input):
//
// frame_corr_kernel: a workgroup owns a tile of 256 decided positions and a halo of W on each
// side. It stages the 256 + 2W + L - 1 symbols and the unique word in LDS once (8-byte entries:
// consecutive lanes read consecutive entries, the unique word is a broadcast), computes m and e for
// tile and halo in the header's order (four accumulators by j mod 4, ascending j, (a0 + a1) +
// (a2 + a3)), keeps m in LDS, and runs the peak test of its tile from there. A thread's first
// position is its tile position, the next two are halo positions, so c and e of a hit are already
// in its registers. The halo is recomputed rather than read back from an m array in HBM: that
// second pass would write and re-read 4 bytes per position (and c, e for the hits) on top of the 8
// bytes of input, one more launch and one more workspace, to save 2W / 256 of the arithmetic, which
// is 12 % at L = W = 16, 50 % at 64 and a factor 3 only at W = 256, where the tile could be widened
// instead. Hits are ranked inside the tile by ballots (ascending position) and their {c, e, offset}
// records written to the tile's own slots, with the tile's hit count.
//
// frame_scan_kernel: one workgroup, sync_scan_kernel's shape: the exclusive prefix sum of the tile
// counts in uint64 (exact), and the total into *count.
//
// frame_emit_kernel: a thread per tile stores pos, phi, metric of its records at off + rank while
// that is below cap; the same launch moves the last `keep` symbols into the handle's other carry
// slot.
//
// frame_gather_kernel: a workgroup per frame row, a lane per group of 4 symbols, 16-byte loads and
// stores where the row is 16-byte aligned, symbol by symbol (or component by component) otherwise.
//
// Plain vector stores only, no atomics, everything indexed at compile time: no scratch. Order and
// bytes do not depend on scheduling.
#include "modem_device.h"
#include "modem_frame_math.h"

namespace mk {

namespace {

constexpr int kFrNT = 256;
constexpr int kFrSlots = 3;              // positions per thread: tile, then up to two of the halo
constexpr int kFrMaxBlocks = 2048;
constexpr int kFrG = 4;                  // symbols per lane and step of the gather
constexpr int kFrScanPer = 4;

typedef uint32_t fv4u __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ T fld(const void* p) {
    return *(const __attribute__((address_space(1))) T*)p;
}
template <typename T> __device__ __forceinline__ void fst(void* p, T v) { *(__attribute__((address_space(1))) T*)p = v; }

__device__ __forceinline__ void fr_unpack_h2(uint32_t w, float& a, float& b) {
    const __half2 h = *reinterpret_cast<const __half2*>(&w);
    a = __low2float(h);
    b = __high2float(h);
}
__device__ __forceinline__ uint32_t fr_pack_h2(float a, float b) {       // round to nearest even
    const __half2 h = __floats2half2_rn(a, b);
    return *reinterpret_cast<const uint32_t*>(&h);
}

// Symbol I/O of one dtype, the accesses of modem_sync.hip's SyncIO: load4 / store4 = the 16-byte
// accesses of 4 symbols, load1 / store1 = one symbol (pair: symbol-aligned, else two component accesses).
template <typename T> struct FrIO;
template <> struct FrIO<float> {
    static constexpr int ssz = 8;
    __device__ static void load4(const char* p, float (&v)[2 * kFrG]) {
        const gv4f a = fld<gv4f>(p), b = fld<gv4f>(p + 16);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    __device__ static void store4(char* p, const float (&v)[2 * kFrG]) {
        fst<gv4f>(p, (gv4f){v[0], v[1], v[2], v[3]});
        fst<gv4f>(p + 16, (gv4f){v[4], v[5], v[6], v[7]});
    }
    __device__ static void load1(const char* p, bool pair, float& re, float& im) {
        if (pair) {
            const gv2f a = fld<gv2f>(p);
            re = a.x; im = a.y;
        } else {
            re = fld<float>(p); im = fld<float>(p + 4);
        }
    }
    __device__ static void store1(char* p, bool pair, float re, float im) {
        if (pair) {
            fst<gv2f>(p, (gv2f){re, im});
        } else {
            fst<float>(p, re); fst<float>(p + 4, im);
        }
    }
};
template <> struct FrIO<__half> {
    static constexpr int ssz = 4;
    __device__ static void load4(const char* p, float (&v)[2 * kFrG]) {
        const fv4u a = fld<fv4u>(p);
        fr_unpack_h2(a.x, v[0], v[1]); fr_unpack_h2(a.y, v[2], v[3]);
        fr_unpack_h2(a.z, v[4], v[5]); fr_unpack_h2(a.w, v[6], v[7]);
    }
    __device__ static void store4(char* p, const float (&v)[2 * kFrG]) {
        fst<fv4u>(p, (fv4u){fr_pack_h2(v[0], v[1]), fr_pack_h2(v[2], v[3]), fr_pack_h2(v[4], v[5]), fr_pack_h2(v[6], v[7])});
    }
    __device__ static void load1(const char* p, bool pair, float& re, float& im) {
        if (pair) {
            fr_unpack_h2(fld<uint32_t>(p), re, im);
        } else {
            fr_unpack_h2((uint32_t)fld<uint16_t>(p) | (uint32_t)fld<uint16_t>(p + 2) << 16, re, im);
        }
    }
    __device__ static void store1(char* p, bool pair, float re, float im) {
        const uint32_t w = fr_pack_h2(re, im);
        if (pair) {
            fst<uint32_t>(p, w);
        } else {
            fst<uint16_t>(p, (uint16_t)w); fst<uint16_t>(p + 2, (uint16_t)(w >> 16));
        }
    }
};

// symbol j of the logical stream carry || in (0 <= j < ncarry + n)
template <typename InT>
__device__ __forceinline__ void frame_load(const FrameParams& p, int64_t j, float& re, float& im) {
    if (j < p.ncarry) FrIO<InT>::load1(static_cast<const char*>(p.carry) + j * FrIO<InT>::ssz, true, re, im);
    else FrIO<InT>::load1(static_cast<const char*>(p.in) + (j - p.ncarry) * FrIO<InT>::ssz, p.in_align >= 1, re, im);
}

template <typename InT>
__global__ __launch_bounds__(kFrNT) void frame_corr_kernel(const FrameParams p) {
#pragma clang fp contract(off)
    __shared__ gv2f s_sym[kFrameTile + 2 * kFrameMaxW + kFrameMaxL - 1];
    __shared__ gv2f s_uw[kFrameMaxL];
    __shared__ float s_m[kFrameTile + 2 * kFrameMaxW];
    __shared__ uint32_t s_wsum[kFrNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = p.L, W = p.W;
    const int64_t nlog = (int64_t)p.ncarry + p.n;
    const int64_t t0 = p.d0 + (int64_t)blockIdx.x * kFrameTile;     // the tile's first position
    const int64_t k0 = t0 - W;                                      // the position of slot 0
    const int nq = kFrameTile + 2 * W, ns = nq + L - 1;
    for (int i = tid; i < ns; i += kFrNT) {
        const int64_t j = k0 + i;
        float re = 0.f, im = 0.f;
        if (j >= 0 && j < nlog) frame_load<InT>(p, j, re, im);
        s_sym[i] = (gv2f){re, im};
    }
    for (int i = tid; i < L; i += kFrNT) s_uw[i] = (gv2f){p.uw[2 * i], p.uw[2 * i + 1]};
    __syncthreads();

    // ordinal o = tid + 256 q: the tile (slot W + o), then the left halo (slot o - 256), then the right
    int slot[kFrSlots];
    bool act[kFrSlots];                                             // wave-uniform
#pragma unroll
    for (int q = 0; q < kFrSlots; ++q) {
        const int o = tid + kFrNT * q, h = o - kFrNT;
        slot[q] = q == 0 ? W + o : h < W ? h : h + kFrameTile;
        act[q] = wave * 64 + kFrNT * q < nq;
        if (o >= nq) slot[q] = 0;                                   // an idle lane of an active wave: reads in bounds
    }
    float cr[kFrSlots][4], ci[kFrSlots][4], en[kFrSlots][4];
#pragma unroll
    for (int q = 0; q < kFrSlots; ++q)
#pragma unroll
        for (int a = 0; a < 4; ++a) cr[q][a] = ci[q][a] = en[q][a] = 0.f;
    const int L4 = L & ~3;
    for (int j = 0; j < L4; j += 4) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const gv2f u = s_uw[j + a];
#pragma unroll
            for (int q = 0; q < kFrSlots; ++q) {
                if (act[q]) {
                    const gv2f r = s_sym[slot[q] + j + a];
                    frame_mac(cr[q][a], ci[q][a], en[q][a], r.x, r.y, u.x, u.y);
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (L4 + a < L) {
            const gv2f u = s_uw[L4 + a];
#pragma unroll
            for (int q = 0; q < kFrSlots; ++q) {
                if (act[q]) {
                    const gv2f r = s_sym[slot[q] + L4 + a];
                    frame_mac(cr[q][a], ci[q][a], en[q][a], r.x, r.y, u.x, u.y);
                }
            }
        }
    }
    float c_re = 0.f, c_im = 0.f, e0 = 0.f, m0 = 0.f;
#pragma unroll
    for (int q = 0; q < kFrSlots; ++q) {
        if (act[q] && tid + kFrNT * q < nq) {
            const int64_t k = k0 + slot[q];
            const float re = frame_join(cr[q]), im = frame_join(ci[q]), e = frame_join(en[q]);
            // a position without all its L symbols does not exist: NaN imposes no condition
            const float m = (k >= 0 && k <= nlog - L) ? frame_mag(re, im) : __builtin_nanf("");
            s_m[slot[q]] = m;
            if (q == 0) { c_re = re; c_im = im; e0 = e; m0 = m; }
        }
    }
    __syncthreads();

    bool hit = t0 + tid < p.d1 && frame_pass(m0, e0, p.t2);
    if (hit) {
        const int c = W + tid;
        for (int d = 1; d <= W; ++d) {
            const float mb = s_m[c - d], ma = s_m[c + d];
            if ((frame_finite(mb) && mb >= m0) || (frame_finite(ma) && ma > m0)) { hit = false; break; }
        }
    }
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) s_wsum[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
    for (int w = 0; w < kFrNT / 64; ++w) {
        if (w < wave) rank += s_wsum[w];
        total += s_wsum[w];
    }
    if (tid == 0) p.cnt[blockIdx.x] = total;
    if (hit && rank < (uint32_t)p.maxh)
        fst<gv4f>(p.rec + 4 * ((int64_t)blockIdx.x * p.maxh + rank), (gv4f){c_re, c_im, e0, __uint_as_float((uint32_t)tid)});
}

__global__ __launch_bounds__(kFrNT) void frame_scan_kernel(const FrameParams p) {
    __shared__ uint64_t wsum[kFrNT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t base = 0;
    for (int64_t c0 = 0; c0 < p.ntiles; c0 += kFrScanPer * kFrNT) {
        const int64_t b0 = c0 + kFrScanPer * tid;
        uint64_t exc[kFrScanPer], run = 0;
#pragma unroll
        for (int j = 0; j < kFrScanPer; ++j) {
            exc[j] = run;
            if (b0 + j < p.ntiles) run += p.cnt[b0 + j];
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
        for (int w = 0; w < kFrNT / 64; ++w) {
            if (w < wave) off += wsum[w];
            tot += wsum[w];
        }
        off += incl - run;
#pragma unroll
        for (int j = 0; j < kFrScanPer; ++j)
            if (b0 + j < p.ntiles) p.off[b0 + j] = off + exc[j];
        base += tot;
        __syncthreads();                                     // wsum is rewritten in the next round
    }
    if (tid == 0) p.count[0] = base;
}

template <typename InT>
__global__ __launch_bounds__(kFrNT) void frame_emit_kernel(const FrameParams p) {
    const int64_t stride = (int64_t)gridDim.x * kFrNT, gid = (int64_t)blockIdx.x * kFrNT + threadIdx.x;
    for (int64_t t = gid; t < p.ntiles; t += stride) {
        const uint32_t n = p.cnt[t] < (uint32_t)p.maxh ? p.cnt[t] : (uint32_t)p.maxh;
        const uint64_t o = p.off[t];
        for (uint32_t r = 0; r < n && o + r < p.cap; ++r) {
            const gv4f v = fld<gv4f>(p.rec + 4 * (t * p.maxh + r));
            const uint64_t i = o + r;
            p.pos[i] = p.base + (uint64_t)(p.d0 + t * kFrameTile) + __float_as_uint(v.w);
            if (p.phi) p.phi[i] = sync_atan2_turn(v.y, v.x);
            if (p.metric) p.metric[i] = frame_metric(frame_mag(v.x, v.y), v.z, p.eu);
        }
    }
    // the last `keep` symbols of the logical stream: into the other carry slot, as values of the input dtype
    const int64_t first = (int64_t)p.ncarry + p.n - p.keep;
    for (int64_t t = gid; t < p.keep; t += stride) {
        float re, im;
        frame_load<InT>(p, first + t, re, im);
        FrIO<InT>::store1(static_cast<char*>(p.carry_new) + t * FrIO<InT>::ssz, true, re, im);
    }
}

template <typename InT, typename OutT>
__global__ __launch_bounds__(kFrNT) void frame_gather_kernel(const FrameGatherParams p) {
    const uint64_t cnt = p.count[0] < p.cap ? p.count[0] : p.cap;
    const int ngroups = (int)((p.len + kFrG - 1) / kFrG);
    for (uint64_t f = blockIdx.x; f < p.cap; f += gridDim.x) {
        bool valid = f < cnt;
        uint64_t first = 0;                                          // the row's first symbol in `in`
        uint32_t rot = 0;
        if (valid) {
            const uint64_t ps = p.pos[f];
            valid = ps <= ~(uint64_t)0 - p.skip && ps + p.skip >= p.base;
            if (valid) {
                first = ps + p.skip - p.base;
                valid = first <= p.n && p.len <= p.n - first;
            }
            if (valid && p.phi && p.lm) rot = frame_rot(p.phi[f], p.lm);
        }
        const char* src = static_cast<const char*>(p.in) + (valid ? first : 0) * FrIO<InT>::ssz;
        char* dst = static_cast<char*>(p.out) + f * p.len * FrIO<OutT>::ssz;
        const bool in_pair = !p.in_elem, out_pair = !p.out_elem;
        const bool in_wide = in_pair && reinterpret_cast<uintptr_t>(src) % 16 == 0;
        const bool out_wide = out_pair && reinterpret_cast<uintptr_t>(dst) % 16 == 0;
        for (int g = threadIdx.x; g < ngroups; g += kFrNT) {
            const uint32_t i0 = (uint32_t)g * kFrG;
            const bool full = i0 + kFrG <= p.len;
            float v[2 * kFrG];
#pragma unroll
            for (int k = 0; k < 2 * kFrG; ++k) v[k] = 0.f;
            if (valid) {
                if (in_wide && full) {
                    FrIO<InT>::load4(src + (size_t)i0 * FrIO<InT>::ssz, v);
                } else {
#pragma unroll
                    for (int k = 0; k < kFrG; ++k)
                        if (i0 + k < p.len) FrIO<InT>::load1(src + (size_t)(i0 + k) * FrIO<InT>::ssz, in_pair, v[2 * k], v[2 * k + 1]);
                }
                if (rot) {
#pragma unroll
                    for (int k = 0; k < kFrG; ++k) frame_rotate(v[2 * k], v[2 * k + 1], rot, p.lm);
                }
            }
            if (out_wide && full) {
                FrIO<OutT>::store4(dst + (size_t)i0 * FrIO<OutT>::ssz, v);
            } else {
#pragma unroll
                for (int k = 0; k < kFrG; ++k)
                    if (i0 + k < p.len) FrIO<OutT>::store1(dst + (size_t)(i0 + k) * FrIO<OutT>::ssz, out_pair, v[2 * k], v[2 * k + 1]);
            }
        }
        if (threadIdx.x == 0) p.ok[f] = valid ? 1 : 0;
    }
}

unsigned frame_grid(int64_t items, int per_block) {
    const int64_t nblk = (items + per_block - 1) / per_block;
    return (unsigned)(nblk < 1 ? 1 : nblk < kFrMaxBlocks ? nblk : kFrMaxBlocks);
}

template <typename InT>
hipError_t frame_go(const FrameParams& p, hipStream_t s) {
    hipError_t e;
    if (p.ntiles > 0) {
        hipLaunchKernelGGL((frame_corr_kernel<InT>), dim3((unsigned)p.ntiles), dim3(kFrNT), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(kFrNT), 0, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.ntiles > 0 || p.keep > 0) {
        hipLaunchKernelGGL((frame_emit_kernel<InT>), dim3(frame_grid(p.ntiles > p.keep ? p.ntiles : p.keep, kFrNT)),
                           dim3(kFrNT), 0, s, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

template <typename InT, typename OutT>
hipError_t frame_gather_go(const FrameGatherParams& p, hipStream_t s) {
    hipLaunchKernelGGL((frame_gather_kernel<InT, OutT>), dim3(frame_grid((int64_t)p.cap, 1)), dim3(kFrNT), 0, s, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_frame(const FrameParams& p0, int in_dtype, hipStream_t s) {
    FrameParams p = p0;
    if (in_dtype != 0 && in_dtype != 1) return hipErrorInvalidValue;
    const int ssz = in_dtype ? 4 : 8;
    const int64_t nlog = (int64_t)p.ncarry + p.n;
    if (p.L < 8 || p.L > kFrameMaxL || p.W < 1 || p.W > kFrameMaxW || p.n < 0 || p.ncarry < 0 ||
        p.ncarry > 2 * p.W + p.L - 1 || p.keep < 0 || p.keep > 2 * p.W + p.L - 1 || p.keep > nlog ||
        p.d0 < 0 || p.d1 < p.d0 || (p.d1 > p.d0 && p.d1 > nlog - p.L + 1) ||
        p.ntiles != (p.d1 - p.d0 + kFrameTile - 1) / kFrameTile || p.ntiles > 0x7fffffff ||
        p.maxh != (kFrameTile + p.W) / (p.W + 1) || !p.count || (p.cap && !p.pos))
        return hipErrorInvalidValue;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p.in);
    if (a % (ssz / 2)) return hipErrorInvalidValue;
    p.in_align = a % ssz == 0 ? 1 : 0;
    return in_dtype ? frame_go<__half>(p, s) : frame_go<float>(p, s);
}

hipError_t launch_frame_gather(const FrameGatherParams& p0, int in_dtype, int out_dtype, hipStream_t s) {
    FrameGatherParams p = p0;
    if ((in_dtype != 0 && in_dtype != 1) || (out_dtype != 0 && out_dtype != 1) || p.lm < 0 || p.lm > 3) return hipErrorInvalidValue;
    if (p.cap == 0) return hipSuccess;
    if (!p.out || !p.ok || !p.pos || !p.count || p.len == 0) return hipErrorInvalidValue;
    const int isz = in_dtype ? 4 : 8, osz = out_dtype ? 4 : 8;
    const uintptr_t ia = reinterpret_cast<uintptr_t>(p.in), oa = reinterpret_cast<uintptr_t>(p.out);
    if (ia % (isz / 2) || oa % (osz / 2)) return hipErrorInvalidValue;
    p.in_elem = ia % isz ? 1 : 0;
    p.out_elem = oa % osz ? 1 : 0;
    switch (in_dtype * 2 + out_dtype) {
    case 0: return frame_gather_go<float, float>(p, s);
    case 1: return frame_gather_go<float, __half>(p, s);
    case 2: return frame_gather_go<__half, float>(p, s);
    default: return frame_gather_go<__half, __half>(p, s);
    }
}

}  // namespace mk
