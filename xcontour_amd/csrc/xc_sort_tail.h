// K8, behind the passes: the block scan, the cumulative area of the sorted state, the sorted values, the profile Q(A) and the
// BPE integral.  Included INSIDE `namespace xc { namespace {` of xc_sort.hip behind xc_sort_key.h.
#pragma once

// exclusive scan in place of row blockIdx.y * gridDim.x + blockIdx.x of `data` (n entries each, one block per row, 1024 entries
// per round behind a carry); TOTALS: the row's sum goes to totals[row].  The radix passes scan every digit's tile counts with it
// (unsigned), the f64 scan below its block sums: the order of the additions is part of k_scan_local's contract.
template <typename T, bool TOTALS>
__global__ __launch_bounds__(1024)
void k_block_exscan(T* __restrict__ data, int n, T* __restrict__ totals)
{
    __shared__ T s_w[16];
    __shared__ T s_carry;
    const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    data += row * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int b = 0; b < n; b += 1024) {
        const int i = b + tid;
        const T v = i < n ? data[i] : (T)0;
        const T x = wave_incl_scan(v, lane);
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        T off = s_carry;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        if (i < n) data[i] = off + x - v;
        __syncthreads();
        if (tid == 1023) s_carry = off + x;
        __syncthreads();
    }
    if (TOTALS && tid == 0) totals[row] = s_carry;
}

// ---- inclusive f64 scan (cumulative area of the sorted state): block sums, their exclusive scan, then
// the block-local scan plus block offset.  Both passes run the same arithmetic, so the sums of pass 1
// are exactly the last values pass 2 produces (read 2x, write 1x; the payload is never re-written).
// A wave owns 512 consecutive values: 4 rounds of coalesced 16-byte accesses, one wave scan per round.
template <bool FINAL>
__global__ __launch_bounds__(256)
void k_scan_local(const double* __restrict__ in, double* __restrict__ out, int64_t n, double* __restrict__ bsum)
{
    __shared__ double s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    in += (size_t)blockIdx.y * n; bsum += (size_t)blockIdx.y * gridDim.x;
    if (FINAL) out += (size_t)blockIdx.y * n;
    const int64_t wbase = (int64_t)blockIdx.x * 2048 + wave * 512;
    double a[4], b[4];
    if (wbase + 512 <= n) {
        const double2* in2 = (const double2*)(in + wbase);
#pragma unroll
        for (int r = 0; r < 4; ++r) { const double2 u = in2[r * 64 + lane]; a[r] = u.x; b[r] = u.y; }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = wbase + (r * 64 + lane) * 2;
            a[r] = i < n ? in[i] : 0.0; b[r] = i + 1 < n ? in[i + 1] : 0.0;
        }
    }
    double carry = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double pair = a[r] + b[r];
        const double x = wave_incl_scan(pair, lane);               // of the pair sums
        const double before = carry + (x - pair);
        a[r] = before + a[r]; b[r] = before + pair;
        carry += __shfl(x, 63);
    }
    if (lane == 63) s_w[wave] = carry;
    __syncthreads();
    double off = 0.0;
    for (int w = 0; w < wave; ++w) off += s_w[w];
    if (FINAL) {
        const double boff = bsum[blockIdx.x];
        if (wbase + 512 <= n) {
            double2* out2 = (double2*)(out + wbase);
#pragma unroll
            for (int r = 0; r < 4; ++r) out2[r * 64 + lane] = make_double2((off + a[r]) + boff, (off + b[r]) + boff);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t i = wbase + (r * 64 + lane) * 2;
                if (i < n) out[i] = (off + a[r]) + boff;
                if (i + 1 < n) out[i + 1] = (off + b[r]) + boff;
            }
        }
    } else if (tid == 255) bsum[blockIdx.x] = off + carry;
}

template <typename K>
__global__ __launch_bounds__(256)
void k_unkey(const K* __restrict__ keys, int64_t n, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    keys += (size_t)blockIdx.y * n; out += (size_t)blockIdx.y * n;
    if (i < n) out[i] = KeyTraits<K>::decode(keys[i]);
}

// Q_exact(A_j) = q_sorted[min(searchsorted(acum[:nvalid], A_j, 'right'), nvalid-1)]
template <typename K>
__device__ __forceinline__ void profile_body(const K* __restrict__ keys, const double* __restrict__ acum,
                                             const unsigned* __restrict__ nvalid, const double* __restrict__ targets, int J,
                                             double* __restrict__ Q, int64_t ncell, int bx)
{
    const int j = bx * 256 + threadIdx.x;
    if (j >= J) return;
    keys += (size_t)blockIdx.y * ncell; acum += (size_t)blockIdx.y * ncell; Q += (size_t)blockIdx.y * J;
    const int64_t n = nvalid[blockIdx.y];
    if (n == 0) { Q[j] = __longlong_as_double(0x7ff8000000000000LL); return; }
    const double a = targets[j];
    int64_t lo = 0, hi = n;                        // first index with acum[idx] > a
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (acum[mid] <= a) lo = mid + 1; else hi = mid; }
    if (lo > n - 1) lo = n - 1;
    Q[j] = KeyTraits<K>::decode(keys[lo]);
}
template <typename K>
__global__ __launch_bounds__(256)
void k_profile(const K* __restrict__ keys, const double* __restrict__ acum,
               const unsigned* __restrict__ nvalid, const double* __restrict__ targets, int J,
               double* __restrict__ Q, int64_t ncell)
{
    profile_body<K>(keys, acum, nvalid, targets, J, Q, ncell, (int)blockIdx.x);
}

// BPE-like integral: sum_i q_i * z*(A_i - dA_i/2) * dA_i with z* = np.interp(A, tbl, coord)
template <typename K>
__global__ __launch_bounds__(256)
void k_bpe(const K* __restrict__ keys, const double* __restrict__ vals,
           const double* __restrict__ acum, const unsigned* __restrict__ nvalid,
           const double* __restrict__ tbl, const double* __restrict__ coord, int ntbl, double* __restrict__ part,
           int64_t ncell, unsigned* __restrict__ tick, double* __restrict__ out,
           const double* __restrict__ targets, int J, double* __restrict__ Q, int nprof)
{
    // (round 5) the first `nprof` workgroups are the profile Q(A_j) of this plane (k_profile's body): both only read the sorted
    // state, so the J binary searches -- ~19 dependent reads, 7 us as a launch of their own -- run beside the integral (cfg5:
    // -6 us, same-box A/B).  Folding a seam into the LAST-ARRIVING workgroup of the kernel before it does NOT pay: tried on the
    // range table (into k_range_hist) and the block-sum scan (into the first scan pass) -- ticket round trip + agent-scope
    // re-reads cost the 3-4 us the launch boundary costs; 3 / 16 / 64-plane stacks +1..3 us, reverted (profiles/r05_notes.md).
    if ((int)blockIdx.x < nprof) { profile_body<K>(keys, acum, nvalid, targets, J, Q, ncell, (int)blockIdx.x); return; }
    const int bx = (int)blockIdx.x - nprof, nbx = (int)gridDim.x - nprof;
    { const size_t so = (size_t)blockIdx.y * ncell; keys += so; vals += so; acum += so; }
    part += (size_t)blockIdx.y * nbx;
    const int64_t n = nvalid[blockIdx.y];
    // the table goes into LDS when it fits (nz or ny entries): the bracket search is a chain of ~log2(ntbl) dependent reads per
    // cell, ~1 us each from global memory (20 us per launch on the cfg5 stand-in), ~0.1 us from LDS
    constexpr int BPE_TBL = 2048;
    __shared__ double s_tbl[2 * BPE_TBL];
    const bool in_lds = ntbl <= BPE_TBL;
    if (in_lds) {
        for (int i = threadIdx.x; i < ntbl; i += 256) { s_tbl[i] = tbl[i]; s_tbl[BPE_TBL + i] = coord[i]; }
        __syncthreads();
    }
    const bool tinc = tbl[ntbl - 1] > tbl[0];
    double sum = 0.0;
    // BU cells per thread and round: their three loads each are issued before the first bracket search starts (one cell at a time --
    // load, ~log2(ntbl) dependent LDS reads, a division, next load -- was a chain of seven memory round trips per thread on the cfg5
    // planes: 19 us for a kernel that moves 32 MB); the terms are still added in cell order
    constexpr int BU = 4;
    auto walk = [&](auto X, auto F) {
        const int64_t step = (int64_t)nbx * 256;
        for (int64_t i0 = (int64_t)bx * 256 + threadIdx.x; i0 < n; i0 += BU * step) {
            double ac[BU], va[BU]; K ke[BU];
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                const int64_t i = i0 + u * step, ic = i < n ? i : n - 1;
                ac[u] = acum[ic]; va[u] = vals[ic]; ke[u] = keys[ic];
            }
#pragma unroll
            for (int u = 0; u < BU; ++u) {
                if (i0 + u * step >= n) break;
                const double a = ac[u] - 0.5 * va[u];
                double z;
                if (a >= X(ntbl - 1)) z = F(ntbl - 1);
                else if (a <= X(0)) z = F(0);
                else {
                    int lo = 0, hi = ntbl - 1;
                    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (a >= X(mid)) lo = mid; else hi = mid; }
                    z = F(lo) + (F(lo + 1) - F(lo)) * (a - X(lo)) / (X(lo + 1) - X(lo));
                }
                sum += KeyTraits<K>::decode(ke[u]) * z * va[u];
            }
        }
    };
    if (in_lds) walk([&](int k) { return s_tbl[tinc ? k : ntbl - 1 - k]; }, [&](int k) { return s_tbl[BPE_TBL + (tinc ? k : ntbl - 1 - k)]; });
    else walk([&](int k) { return tinc ? tbl[k] : tbl[ntbl - 1 - k]; }, [&](int k) { return tinc ? coord[k] : coord[ntbl - 1 - k]; });
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = sum;
    __syncthreads();
    // (round 5) the block that arrives last sums the plane's partials in block order -- one launch less at the end of the chain.  Every
    // hand-off word is an agent-scope 8-byte atomic on both sides (a partial is ONE store of one lane, the ticket returns the order of
    // arrival): MI355X_MICROARCH.md, valid forms; the sum is taken in a fixed order, whoever arrives last.
    __shared__ unsigned s_last;
    if (threadIdx.x == 0) {
        __hip_atomic_store(part + bx, s[0] + s[1] + s[2] + s[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = __hip_atomic_fetch_add(tick + (size_t)blockIdx.y * 4, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nbx - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= 64) return;
    const int np = nbx, per = (np + 63) / 64, i0 = (int)threadIdx.x * per;     // one wave: lane l sums its contiguous share, then a fixed xor tree
    double t = 0.0;
    for (int i = i0; i < i0 + per && i < np; ++i) t += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (threadIdx.x == 0) {
        out[blockIdx.y] = t;
        __hip_atomic_store(tick + (size_t)blockIdx.y * 4, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch (a stack that is sorted again runs this kernel twice)
    }
}
