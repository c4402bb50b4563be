// K13's fixed-point sums, shared by K13 (xc_cpiece.hip) and K17 (xc_cinside.hip); xc_cpiece.hip's header states the rule: every term is
// added WHOLE to CP_L 32-bit limbs kept in 64-bit words, the words are carried and rounded once (half to even), so a sum is the exact
// sum of its terms whatever the order of arrival.  A word takes 2^31 chunks before it could wrap.  Included inside
// namespace xc { namespace { ... } } after xc_binning.h.
#pragma once

constexpr int CP_L = 5;                       // 32-bit limbs per accumulator: a 160-bit window, 148 bits of it below the bound

// the top exponent of the window from a window constant of det_c0_from_bound
__device__ __forceinline__ int cp_top(int c0) { return c0 - (1023 + 52 - (53 - kDetPrecBits)); }

// One term cut at the limb boundaries (limb j counts units of 2^(top - 32 (j + 1))): chunk t of c[] (each below 2^32) belongs to limb
// CP_L - 1 - k - t, negated where `neg`.  Returns 0 when the term adds nothing (zeros and denormals lie under every window, and so may
// the whole term), 2 when it is not finite, else 1.  Bits under the window's bottom are dropped: a function of the term alone.
__device__ __forceinline__ int cp_split(double v, int top, unsigned long long (&c)[3], int& k, bool& neg)
{
    const unsigned bh = (unsigned)__double2hiint(v), bl = (unsigned)__double2loint(v);
    const int Eb = (int)((bh >> 20) & 0x7ffu);
    if (Eb == 2047) return 2;
    if (Eb == 0) return 0;
    unsigned long long m = ((unsigned long long)((bh & 0xfffffu) | 0x100000u) << 32) | bl;
    neg = (bh >> 31) != 0u;
    int sh = (Eb - 1075) - (top - 32 * CP_L);                              // bits between m's last bit and the window's bottom
    if (sh < 0) {
        if (sh <= -53) return 0;
        m >>= -sh; sh = 0;
    }
    const int s = sh & 31;
    k = sh >> 5;
    const unsigned long long lo = m << s, hi = s ? m >> (64 - s) : 0ull;
    c[0] = lo & 0xffffffffull; c[1] = lo >> 32; c[2] = hi;
    return 1;
}

// one term, whole, into the CP_L words of its accumulator in memory: one 64-bit integer atomic per non-zero chunk
__device__ __forceinline__ void cp_add(unsigned long long* __restrict__ acc, int* __restrict__ flag, int bit, double v, int top)
{
    unsigned long long c[3]; int k = 0; bool neg = false;
    const int st = cp_split(v, top, c, k, neg);
    if (st == 2) { atomicOr(flag, bit); return; }
    if (st == 0) return;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (c[t] == 0ull) continue;
        const int j = CP_L - 1 - k - t;
        if (j < 0) { atomicOr(flag, bit); continue; }                      // above the window: the term broke its bound
        atomicAdd(acc + j, neg ? (unsigned long long)(-(long long)c[t]) : c[t]);
    }
}

// the same into CP_L words a thread keeps in registers (no limb is indexed by a run-time value); returns false where cp_add would flag
__device__ __forceinline__ bool cp_add_private(unsigned long long (&acc)[CP_L], double v, int top)
{
    unsigned long long c[3]; int k = 0; bool neg = false;
    const int st = cp_split(v, top, c, k, neg);
    if (st == 2) return false;
    if (st == 0) return true;
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int j = CP_L - 1 - k - t;
        const unsigned long long a = neg ? (unsigned long long)(-(long long)c[t]) : c[t];
        if (j < 0) ok = ok && c[t] == 0ull;
#pragma unroll
        for (int l = 0; l < CP_L; ++l) acc[l] += l == j ? a : 0ull;
    }
    return ok;
}

// the words of an accumulator (signed sums of chunks), carried and converted ONCE: round half to even
__device__ __forceinline__ double cp_to_double(const unsigned long long* __restrict__ acc, int top)
{
    long long w[CP_L];
#pragma unroll
    for (int j = 0; j < CP_L; ++j) w[j] = (long long)acc[j];
#pragma unroll
    for (int j = CP_L - 1; j > 0; --j) { const long long c = w[j] >> 32; w[j] -= c << 32; w[j - 1] += c; }
    const bool neg = w[0] < 0;
    if (neg) {
        long long borrow = 0;
#pragma unroll
        for (int j = CP_L - 1; j >= 0; --j) {
            long long t = -w[j] - borrow; borrow = 0;
            if (j > 0 && t < 0) { t += 1ll << 32; borrow = 1; }
            w[j] = t;
        }
    }
    constexpr int ND = CP_L + 1;                                           // 32-bit digits: the top word gives two
    unsigned long long d[ND];
    d[0] = (unsigned long long)w[0] >> 32; d[1] = (unsigned long long)w[0] & 0xffffffffull;
#pragma unroll
    for (int j = 1; j < CP_L; ++j) d[j + 1] = (unsigned long long)w[j];
    int first = -1;
#pragma unroll
    for (int i = 0; i < ND; ++i) if (first < 0 && d[i] != 0ull) first = i;
    if (first < 0) return 0.0;
    unsigned long long T = 0ull; int nb = 0, below = 0; bool sticky = false;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        const unsigned long long D = d[i];
        if (i == first) { T = D; nb = 64 - __clzll((long long)D); below = 32 * (ND - 1 - i); }
        else if (i > first) {
            if (nb + 32 <= 64) { T = (T << 32) | D; nb += 32; below -= 32; }
            else if (nb < 64) {
                const int take = 64 - nb, rest = 32 - take;
                T = (T << take) | (D >> rest);
                sticky = sticky || (D & ((1ull << rest) - 1ull)) != 0ull;
                nb = 64; below -= take;
            } else sticky = sticky || D != 0ull;
        }
    }
    int e = (top - 32 * CP_L) + below;
    if (nb > 53) {
        const int drop = nb - 53;
        const unsigned long long rem = T & ((1ull << drop) - 1ull), half = 1ull << (drop - 1);
        T >>= drop;
        if (rem > half || (rem == half && (sticky || (T & 1ull)))) ++T;
        e += drop;
    }
    const double out = ldexp((double)T, e);
    return neg ? -out : out;
}
