// rust-modem_amd/csrc/modem_ratematch.hip — rate matching (puncturing and a pruned block
// interleaver) and the frame check (a CRC), no reference counterpart; include/modem_hip.h, "Rate
// matching and frame check". The integer rules are modem_ratematch_math.h.
//
// rm_rx_kernel<T>: a workgroup takes a group of G frames (as many as 64 KiB of LDS hold, at most
// kRmMaxGroup, and no more than make about kRmGroupElems outputs: short frames share a workgroup).
// It loads each frame's E transmitted values into LDS, consecutive lanes on consecutive elements,
// meets at a barrier, and then lane by lane takes mother index m, works out pi(rank(m)) once (a
// division by P, a popcount of the pattern mask, a division by C) and stores that element of every
// frame of the group: consecutive lanes store consecutive m, 64 elements per store, and the
// strided side of the permutation is an LDS read. Values move as bits (T is an unsigned integer of
// the element's size); a punctured m gets 0.
// rm_tx_kernel: the mirror on bytes: a coalesced load of in[f][m], a scatter into LDS at
// pi(rank(m)) (every cell of the E is written once: pi o rank is a bijection), a barrier, and a
// linear store of the E bytes.
// crc_kernel<Attach>: a wave per frame, kCrcWaves frames per workgroup, no barrier. Lane l runs the
// bit steps over chunk l of the row (64 chunks of ceil(L / 64) bits, aligned to the row's end), and
// six joins over shuffles fold the 64 registers: at distance d the left register is multiplied by
// x^(d len) mod poly, a power that is the same for the whole launch and is squared from level to
// level before the frame loop. Attach copies the bits and appends the W bits; check compares the W
// trailing bits under one ballot and writes ok.
//
// Plain vector loads and stores only, no atomics, no global workspace, no scratch. The grids are
// capped and loop with a grid stride.
#include "modem_device.h"
#include "modem_ratematch_math.h"

namespace mk {

namespace {

constexpr int kRmNT = 256;
constexpr int kRmMaxBlocks = 1024;
constexpr int kRmMaxGroup = 16;                  // frames a workgroup takes at a time
constexpr int kRmGroupElems = 4096;              // outputs of a group, about: short frames share a workgroup
constexpr int kRmLds = 65536;                    // LDS a workgroup may ask for
constexpr int kCrcWaves = 4;                     // frames per workgroup and trip, a wave each
constexpr int kCrcMaxBlocks = 1024;

template <typename T>
__global__ __launch_bounds__(kRmNT) void rm_rx_kernel(const RmParams p, const uint32_t G) {
    extern __shared__ uint32_t rm_lds[];
    T* buf = reinterpret_cast<T*>(rm_lds);
    const T* in = static_cast<const T*>(p.in);
    T* out = static_cast<T*>(p.out);
    const uint64_t ngroups = (p.nframes + G - 1) / G;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t f0 = g * G;
        const uint32_t nf = p.nframes - f0 < G ? (uint32_t)(p.nframes - f0) : G;
        for (uint32_t fi = 0; fi < nf; ++fi) {
            const T* row = in + (f0 + fi) * p.in_stride;
            for (uint32_t j = threadIdx.x; j < p.E; j += kRmNT) buf[fi * p.E + j] = row[j];
        }
        __syncthreads();
        for (uint32_t m = threadIdx.x; m < p.nm; m += kRmNT) {
            const bool kept = rm_is_kept(p.mask, p.P, m);
            const uint32_t q = kept ? rm_pi(rm_rank(p.mask, p.P, p.w, m), p.C, p.rows, p.cl) : 0u;
            for (uint32_t fi = 0; fi < nf; ++fi) out[(f0 + fi) * p.out_stride + m] = kept ? buf[fi * p.E + q] : (T)0;
        }
        __syncthreads();                                // the next trip overwrites the group's values
    }
}

__global__ __launch_bounds__(kRmNT) void rm_tx_kernel(const RmParams p, const uint32_t G) {
    extern __shared__ uint32_t rm_lds[];
    uint8_t* buf = reinterpret_cast<uint8_t*>(rm_lds);
    const uint8_t* in = static_cast<const uint8_t*>(p.in);
    uint8_t* out = static_cast<uint8_t*>(p.out);
    const uint64_t ngroups = (p.nframes + G - 1) / G;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t f0 = g * G;
        const uint32_t nf = p.nframes - f0 < G ? (uint32_t)(p.nframes - f0) : G;
        for (uint32_t m = threadIdx.x; m < p.nm; m += kRmNT) {
            if (!rm_is_kept(p.mask, p.P, m)) continue;
            const uint32_t q = rm_pi(rm_rank(p.mask, p.P, p.w, m), p.C, p.rows, p.cl);
            for (uint32_t fi = 0; fi < nf; ++fi) buf[fi * p.E + q] = in[(f0 + fi) * p.in_stride + m] & 1u;
        }
        __syncthreads();
        for (uint32_t fi = 0; fi < nf; ++fi) {
            uint8_t* row = out + (f0 + fi) * p.out_stride;
            for (uint32_t j = threadIdx.x; j < p.E; j += kRmNT) row[j] = buf[fi * p.E + j];
        }
        __syncthreads();
    }
}

// Frames of a group: LDS holds E elements of `elem` bytes for each.
uint32_t rm_group(const RmParams& p, int elem) {
    uint64_t G = (uint64_t)kRmLds / ((uint64_t)p.E * elem);
    const uint64_t want = (uint64_t)kRmGroupElems / p.nm;
    if (G > want) G = want;
    if (G > (uint64_t)kRmMaxGroup) G = kRmMaxGroup;
    if (G > p.nframes) G = p.nframes;
    return G < 1 ? 1u : (uint32_t)G;
}

bool rm_params_ok(const RmParams& p) {
    if (p.P < 1 || p.P > (uint32_t)kRmMaxP || p.C < 1 || p.C > (uint32_t)kRmMaxCols || p.nm < 1 || p.nm > (uint32_t)kRmMaxNm) return false;
    if (p.P < 64 && (p.mask >> p.P)) return false;
    if (p.w != rm_popcount(p.mask) || p.w < 1 || p.E != rm_kept(p.mask, p.P, p.nm) || p.E < 1) return false;
    return p.rows == rm_rows(p.E, p.C) && p.cl == p.E - (p.rows - 1) * p.C;
}

template <bool Attach>
__global__ __launch_bounds__(64 * kCrcWaves) void crc_kernel(const CrcParams p) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t W = p.W, poly = p.poly, L = p.nbits;
    // x^(d len), d = 1, 2, 4 .. 32: what the left register of a join at distance d is multiplied by
    uint32_t xp[6];
    xp[0] = crc_xpow(crc_chunk_len(L), W, poly);
#pragma unroll
    for (int k = 1; k < 6; ++k) xp[k] = crc_mul(xp[k - 1], xp[k - 1], W, poly);
    const uint64_t stride = (uint64_t)gridDim.x * kCrcWaves;
    for (uint64_t f = (uint64_t)blockIdx.x * kCrcWaves + wave; f < p.nframes; f += stride) {
        const uint8_t* row = p.in + f * p.in_stride;
        uint32_t v = crc_chunk_reg(L, lane, W, poly, p.init, [row](uint32_t i) { return (uint32_t)row[i]; });
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t right = (uint32_t)__shfl_down((int)v, 1u << k, 64);
            v = crc_join(v, right, xp[k], W, poly);     // lanes that are multiples of 2^(k+1) hold whole blocks
        }
        const uint32_t crc = (uint32_t)__shfl((int)v, 0, 64) ^ p.xorout;
        if (Attach) {
            uint8_t* o = p.out + f * p.out_stride;
            for (uint32_t i = lane; i < L; i += 64) o[i] = row[i] & 1u;
            if (lane < W) o[L + lane] = (uint8_t)((crc >> (W - 1 - lane)) & 1u);
        } else {
            const bool bad = lane < W && (uint32_t)(row[L + lane] & 1u) != ((crc >> (W - 1 - lane)) & 1u);
            const uint64_t anybad = __ballot(bad);
            if (lane == 0) p.out[f] = (uint8_t)(anybad == 0 && (!p.ok_in || p.ok_in[f] != 0));
        }
    }
}

bool crc_params_ok(const CrcParams& p) {
    if (p.W != 8 && p.W != 16 && p.W != 24 && p.W != 32) return false;
    const uint32_t mask = crc_mask(p.W);
    if ((p.poly | p.init | p.xorout) & ~mask) return false;
    return p.nbits >= 1 && p.nbits <= (uint32_t)kCrcMaxBits && p.in_stride >= (uint64_t)p.nbits;
}

template <bool Attach>
hipError_t crc_go(const CrcParams& p, hipStream_t s) {
    const uint64_t nblk = (p.nframes + kCrcWaves - 1) / kCrcWaves;
    hipLaunchKernelGGL(crc_kernel<Attach>, dim3((unsigned)(nblk < (uint64_t)kCrcMaxBlocks ? nblk : (uint64_t)kCrcMaxBlocks)),
                       dim3(64 * kCrcWaves), 0, s, p);
    return hipGetLastError();
}

unsigned rm_blocks(uint64_t nframes, uint32_t G) {
    const uint64_t ngroups = (nframes + G - 1) / G;
    return (unsigned)(ngroups < (uint64_t)kRmMaxBlocks ? ngroups : (uint64_t)kRmMaxBlocks);
}

}  // namespace

hipError_t launch_rm_tx(const RmParams& p, hipStream_t s) {
    if (!rm_params_ok(p) || p.in_stride < p.nm || p.out_stride < p.E) return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.in || !p.out) return hipErrorInvalidValue;
    const uint32_t G = rm_group(p, 1);
    hipLaunchKernelGGL(rm_tx_kernel, dim3(rm_blocks(p.nframes, G)), dim3(kRmNT), (size_t)G * p.E, s, p, G);
    return hipGetLastError();
}

hipError_t launch_rm_rx(const RmParams& p, int elem, hipStream_t s) {
    if (!rm_params_ok(p) || p.in_stride < p.E || p.out_stride < p.nm || (elem != 1 && elem != 2 && elem != 4)) return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.in || !p.out) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(p.in) | reinterpret_cast<uintptr_t>(p.out)) % (uintptr_t)elem) return hipErrorInvalidValue;
    const uint32_t G = rm_group(p, elem);
    const dim3 grid(rm_blocks(p.nframes, G)), block(kRmNT);
    const size_t lds = (size_t)G * p.E * elem;
    switch (elem) {
    case 1: hipLaunchKernelGGL(rm_rx_kernel<uint8_t>, grid, block, lds, s, p, G); break;
    case 2: hipLaunchKernelGGL(rm_rx_kernel<uint16_t>, grid, block, lds, s, p, G); break;
    default: hipLaunchKernelGGL(rm_rx_kernel<uint32_t>, grid, block, lds, s, p, G); break;
    }
    return hipGetLastError();
}

hipError_t launch_crc_attach(const CrcParams& p, hipStream_t s) {
    if (!crc_params_ok(p) || p.out_stride < (uint64_t)p.nbits + p.W) return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.in || !p.out) return hipErrorInvalidValue;
    return crc_go<true>(p, s);
}

hipError_t launch_crc_check(const CrcParams& p, hipStream_t s) {
    if (!crc_params_ok(p) || p.in_stride < (uint64_t)p.nbits + p.W) return hipErrorInvalidValue;
    if (p.nframes == 0) return hipSuccess;
    if (!p.in || !p.out) return hipErrorInvalidValue;
    return crc_go<false>(p, s);
}

}  // namespace mk
