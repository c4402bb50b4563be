// K13's root and slot numbering, shared by K13 (xc_cpiece.hip) and K18-K21 (xc_cprecords.hip); xc_cpiece.hip's header states the rule: after
// phase A (xc_cpiece_link.h) a segment that is its own root takes the next slot of its range and notes whether its piece is open.
// Included inside namespace xc { namespace { ... } } after xc_cpiece_link.h.
#pragma once

constexpr int CP_OPEN = (int)0x80000000u;     // slot: the piece is open

// roots take their slots: root[i] (group-local) for every segment, slot[i] (with the open bit) for roots only
__global__ __launch_bounds__(CP_TPB)
void k_cp_root(int64_t n, long long E, const int* __restrict__ tab, const int* __restrict__ rid, const int* __restrict__ lab,
               const int* __restrict__ prv, int64_t r0, unsigned long long* __restrict__ piece_count, int* __restrict__ root,
               int* __restrict__ slot)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    const bool valid = i < n;
    int r = -1;
    bool isroot = false;
    if (valid) {
        r = rid[i];
        const int l = lab[i];
        int t = (l >= 0 && l < E) ? tab[(size_t)r * E + l] : (int)i;
        if (t < 0 || t >= n) t = (int)i;
        root[i] = t;
        isroot = t == (int)i;
    }
    const int rf = __builtin_amdgcn_readfirstlane(r);
    const int lane = threadIdx.x & 63;
    int s = 0;
    if (__all(!valid || r == rf)) {                                   // the wave lies in one range: one atomic for all its roots
        const unsigned long long m = __ballot(isroot);
        if (m != 0ull) {
            int base = 0;
            if (lane == 0) base = (int)atomicAdd(piece_count + r0 + rf, (unsigned long long)__popcll(m));
            base = __shfl(base, 0);
            s = base + __popcll(m & ((1ull << lane) - 1ull));
        }
    } else if (isroot) {
        s = (int)atomicAdd(piece_count + r0 + r, 1ull);
    }
    if (isroot) slot[i] = s | (prv[i] < 0 ? CP_OPEN : 0);
}
