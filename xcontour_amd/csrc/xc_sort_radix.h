// K8, the radix passes: tile histogram and scatter of one LSD pass, the repair of the range-key runs, the count of the valid
// cells.  Included INSIDE `namespace xc { namespace {` of xc_sort.hip behind xc_sort_key.h; FIX_* are defined there.
#pragma once

// peer mask of lanes holding the same 8-bit digit (only lanes in `valid`)
__device__ __forceinline__ unsigned long long digit_peers(unsigned d, unsigned long long valid)
{
    unsigned long long m = valid;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const unsigned long long bal = __ballot((d >> b) & 1u);
        m &= ((d >> b) & 1u) ? bal : ~bal;
    }
    return m;
}

// one key of a round into the wave's counters; a round of a `full` part whose 64 digits are all equal -- sorted or constant
// data -- is added once by one lane
__device__ __forceinline__ void count_digit(unsigned* cnt, unsigned d, bool full, bool valid, int lane)
{
    const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)d);
    if (full && __ballot(d != d0) == 0ull) { if (lane == 0) atomicAdd(&cnt[d0], 64u); }
    else if (valid) atomicAdd(&cnt[d], 1u);
}

// tile = 4 waves x TILE elements (one block); digit-major tile histogram hist[d][tile].
// Counting needs no ranks: one returnless ds_add_u32 per key on per-wave counters (the ballot ranking
// of the scatter costs ~60 VALU instructions per 64 keys and made this kernel ALU-bound).
template <typename K, bool FIRST, typename TQ, typename TM, int MODE, int TR>
__global__ __launch_bounds__(256)
void k_radix_hist(const K* __restrict__ keys, int64_t n, int shift, int ntiles, unsigned* __restrict__ hist, const PairSrc src)
{
    constexpr int TILE_ROUNDS = TR, TILE = 64 * TR, BTILE = 4 * TILE;      // (the tile of THIS instance: small_tiles() in xc_sort.hip)
    __shared__ unsigned s_cnt[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = blockIdx.x;
    __shared__ unsigned s_rt[MODE == 1 ? 2 * RANGE_NB : 1];
    RangeMap rm = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr};
    if (MODE == 1) rm = range_map(src, blockIdx.y, s_rt);
    keys += (size_t)blockIdx.y * n; hist += (size_t)blockIdx.y * 256 * ntiles;
    for (int i = lane; i < 256; i += 64) s_cnt[wave][i] = 0;
    if (MODE == 1) __syncthreads();
    // counting does not care about the order inside the tile: register r of a lane holds cell base + ((r / KPL) * 64 + lane) * KPL + r % KPL
    constexpr int KPL = FIRST ? 1 : 16 / (int)sizeof(K);
    const int64_t base = t * BTILE + (int64_t)wave * TILE;
    K kreg[TILE_ROUNDS];                                   // all loads of the wave's part in flight at once
    const bool full = base + TILE <= n;
    if constexpr (FIRST) {
        // pass 0: the keys do not exist yet -- encode them from the tracer
        const TQ* q = (const TQ*)src.q + (size_t)blockIdx.y * n;
        const TM* mask = src.mask ? (const TM*)src.mask + (size_t)blockIdx.y * src.mask_stride : nullptr;
        double dummy[TILE_ROUNDS];
        load_pairs<TQ, TM, K, TILE_ROUNDS, false>(q, mask, nullptr, XC_DA_NONE, src.nx, src.negate, base, lane, n, kreg, dummy);
    } else if (full) {
        // 16-byte loads, KPL keys per lane and load
        struct alignas(16) Pack { K k[KPL]; };
        const Pack* kp = (const Pack*)(keys + base);       // workspace is 256-byte aligned, base a multiple of 1024
#pragma unroll
        for (int r = 0; r < TILE_ROUNDS / KPL; ++r) {
            const Pack u = kp[r * 64 + lane];
#pragma unroll
            for (int c = 0; c < KPL; ++c) kreg[KPL * r + c] = u.k[c];
        }
    } else {
#pragma unroll
        for (int r = 0; r < TILE_ROUNDS / KPL; ++r)
#pragma unroll
            for (int c = 0; c < KPL; ++c) {
                const int64_t i = base + (int64_t)(r * 64 + lane) * KPL + c;
                kreg[KPL * r + c] = i < n ? keys[i] : (K)0;
            }
    }
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int64_t i = base + (int64_t)((r / KPL) * 64 + lane) * KPL + (r % KPL);
        count_digit(s_cnt[wave], digit_of<K, MODE>(kreg[r], shift, rm), full, (!FIRST && full) || i < n, lane);
    }
    __syncthreads();
    const int d = threadIdx.x;
    hist[(size_t)d * ntiles + t] = s_cnt[0][d] + s_cnt[1][d] + s_cnt[2][d] + s_cnt[3][d];
}


// Scatter of one block tile (4 waves x TILE elements).  The tile is first sorted by digit in LDS
// (stable: wave-major, then round, then lane = element order), then written out position by position:
// consecutive LDS positions with the same digit go to consecutive global addresses, so the stores
// of a wave cover runs of ~BTILE/256 elements instead of 64 unrelated 8-byte targets.
template <typename K, bool FIRST, typename TQ, typename TM, int MODE, int TR>
__global__ __launch_bounds__(256)
void k_radix_scatter(const K* __restrict__ kin, const double* __restrict__ vin,
                     K* __restrict__ kout, double* __restrict__ vout, int64_t n, int shift,
                     int ntiles, const unsigned* __restrict__ hist, const unsigned* __restrict__ totals, int inline_scan,
                     const PairSrc src)
{
    constexpr int TILE_ROUNDS = TR, TILE = 64 * TR, BTILE = 4 * TILE;
    extern __shared__ unsigned long long s_dyn[];
    K* s_k = (K*)s_dyn;                                        // [BTILE] staging: keys first, then the payload
    double* s_v = (double*)s_dyn;
    unsigned* s_cnt = (unsigned*)(s_dyn + BTILE);              // [4][256] per-wave digit counts -> start offsets
    unsigned* s_gbase = s_cnt + 4 * 256;                       // [256] global position minus tile-local position
    unsigned* s_wsum = s_gbase + 256;                          // [8]
    unsigned char* s_dig = (unsigned char*)(s_wsum + 8);       // [BTILE] digit of the element at every tile-local position
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t = blockIdx.x;
    __shared__ unsigned s_rt[MODE == 1 ? 2 * RANGE_NB : 1];
    RangeMap rm = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr};
    if (MODE == 1) { rm = range_map(src, blockIdx.y, s_rt); __syncthreads(); }
    { const size_t so = (size_t)blockIdx.y * n; kin += so; vin += so; kout += so; vout += so; }
    hist += (size_t)blockIdx.y * 256 * ntiles; totals += (size_t)blockIdx.y * 256;
    for (int d = lane; d < 256; d += 64) s_cnt[wave * 256 + d] = 0;
    const int64_t tbase = t * BTILE;
    const int64_t base = tbase + (int64_t)wave * TILE;
    K kreg[TILE_ROUNDS];                                       // the whole part's loads in flight at once
    double vreg[TILE_ROUNDS];
    unsigned short lrank[TILE_ROUNDS];
    unsigned char dreg[TILE_ROUNDS];                           // the digit, computed once (the range key costs ~10 VALU operations)
    if constexpr (FIRST) {
        // pass 0 builds its pairs from the tracer / mask / dA (kin / vin do not exist yet; their slab offset above is harmless)
        const TQ* q = (const TQ*)src.q + (size_t)blockIdx.y * n;
        const TM* mask = src.mask ? (const TM*)src.mask + (size_t)blockIdx.y * src.mask_stride : nullptr;
        const double* dA = src.dA ? src.dA + (size_t)blockIdx.y * src.dA_stride : nullptr;
        load_pairs<TQ, TM, K, TILE_ROUNDS, true>(q, mask, dA, src.dA_rank, src.nx, src.negate, base, lane, n, kreg, vreg);
    } else {
#pragma unroll
        for (int r = 0; r < TILE_ROUNDS; ++r) {
            const int64_t i = base + r * 64 + lane;
            kreg[r] = i < n ? kin[i] : (K)0;
            vreg[r] = i < n ? vin[i] : 0.0;
        }
    }
    // rank of every element among the wave's elements with the same digit
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + lane;
        const bool valid = i < n;
        const unsigned d = valid ? digit_of<K, MODE>(kreg[r], shift, rm) : 0u;
        dreg[r] = (unsigned char)d;
        const unsigned long long peers = digit_peers(d, __ballot(valid));
        const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        unsigned pos = 0;
        if (valid) pos = s_cnt[wave * 256 + d] + rank;          // all peers read the same counter first ...
        if (valid && rank == 0) s_cnt[wave * 256 + d] += (unsigned)__popcll(peers);   // ... then the leader advances it
        lrank[r] = (unsigned short)pos;
    }
    __syncthreads();
    {   // thread d: tile-local start of digit d (exclusive scan over digits), per-wave starts, global base
        const int d = tid;
        const unsigned c0 = s_cnt[d], c1 = s_cnt[256 + d], c2 = s_cnt[512 + d], c3 = s_cnt[768 + d];
        // few tiles per plane (stacks of small planes): the scan over the tiles is done right here on the raw counts,
        // the separate row-scan launch (one 1024-thread block per digit and plane) is skipped
        unsigned gtot, before = 0;
        if (inline_scan) {
            gtot = 0;
            for (int tt = 0; tt < ntiles; ++tt) { const unsigned c = hist[(size_t)d * ntiles + tt]; gtot += c; before += tt < t ? c : 0u; }
        } else { gtot = totals[d]; before = hist[(size_t)d * ntiles + t]; }
        const unsigned tot = c0 + c1 + c2 + c3;
        unsigned x = tot, gx = gtot;                       // two exclusive scans over the digits, tile-local and global, in step
        for (int o = 1; o < 64; o <<= 1) {                 // (one loop, not two wave_incl_scan: the hot kernel's code stays as it was)
            const unsigned y = __shfl_up(x, o), gy = __shfl_up(gx, o);
            if (lane >= o) { x += y; gx += gy; }
        }
        if (lane == 63) { s_wsum[wave] = x; s_wsum[4 + wave] = gx; }
        __syncthreads();
        unsigned start = x - tot, gbase = gx - gtot;
        for (int w = 0; w < wave; ++w) { start += s_wsum[w]; gbase += s_wsum[4 + w]; }
        s_cnt[d] = start; s_cnt[256 + d] = start + c0; s_cnt[512 + d] = start + c0 + c1; s_cnt[768 + d] = start + c0 + c1 + c2;
        s_gbase[d] = gbase + before - start;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + lane;
        const unsigned d = dreg[r];
        lrank[r] = (unsigned short)(s_cnt[wave * 256 + d] + lrank[r]);      // tile-local position
        if (i < n) { s_k[lrank[r]] = kreg[r]; s_dig[lrank[r]] = dreg[r]; }
    }
    __syncthreads();
    const int64_t left = n - tbase;
    const int cnt = left < BTILE ? (int)left : BTILE;
    unsigned gpos[TILE_ROUNDS];
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int p = r * 256 + tid;
        if (p < cnt) {
            const K key = s_k[p];
            gpos[r] = s_gbase[s_dig[p]] + (unsigned)p;
            kout[gpos[r]] = key;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int64_t i = base + r * 64 + lane;
        if (i < n) s_v[lrank[r]] = vreg[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TILE_ROUNDS; ++r) {
        const int p = r * 256 + tid;
        if (p < cnt) vout[gpos[r]] = s_v[p];
    }
}

// ---- after the three range-key passes: finish every run of equal range key that is out of order, and count the valid
// cells.  IN PLACE; one block per FIX_C consecutive positions [a, b) OWNS the runs whose first cell (head) lies there, to
// their end -- a run belongs to exactly one block; the block's window is [a - 1, a - 1 + FIX_W).
//   1. head[i] / end[i] of the run of every window cell: a prefix-max / suffix-min scan over the head positions.
//   2. Every inversion (a cell whose full key is smaller than its left neighbour's inside one run) marks its run dirty;
//      if that run is owned and longer than FIX_RUN the flag sends the whole stack to the eight-pass path.  Runs without
//      an inversion -- ties of any length -- are never touched.
//   3. Every cell of a dirty owned run counts the cells of its run that sort before it (smaller key, or equal key and
//      earlier position: a stable rank, at most FIX_RUN reads, ~2 on average) and, if its place changes, writes ITSELF
//      (key and payload from its registers) to head + rank.  The writes of a run are a permutation of the run; a
//      neighbouring block reading such a cell meanwhile only derives its range key from it, which the run shares.
//   The step from the last valid key to the first dropped one (always a head) gives nvalid.
template <typename K>
__global__ __launch_bounds__(256)
void k_fix_runs(K* __restrict__ keys, double* __restrict__ vals, int64_t n, unsigned* __restrict__ flag,
                unsigned* __restrict__ nvalid, const PairSrc src)
{
    __shared__ K s_k[FIX_W];
    __shared__ unsigned s_d[FIX_W];
    __shared__ unsigned short s_h[FIX_W], s_e[FIX_W];
    __shared__ unsigned char s_dirty[FIX_W];
    __shared__ int s_wh[4], s_we[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ unsigned s_rt[2 * RANGE_NB];
    const RangeMap rm = range_map(src, blockIdx.y, s_rt);
    keys += (size_t)blockIdx.y * n; vals += (size_t)blockIdx.y * n;
    const int64_t a = (int64_t)blockIdx.x * FIX_C, w0 = a - 1;               // window position i <-> cell w0 + i; owned heads: i in [1, FIX_C]
    K kr[FIX_NL]; double vr[FIX_NL];                                          // every load issued before the first use
#pragma unroll
    for (int c = 0; c < FIX_NL; ++c) {
        int64_t g = w0 + tid + 256 * c;
        g = g < 0 ? 0 : (g < n ? g : n - 1);
        kr[c] = keys[g]; vr[c] = vals[g];
    }
    __syncthreads();                                                           // the range table is in LDS
#pragma unroll
    for (int c = 0; c < FIX_NL; ++c) {
        const int i = tid + 256 * c;
        const int64_t g = w0 + i;
        const bool in = g >= 0 && g < n;
        s_k[i] = in ? kr[c] : (K)0;
        s_d[i] = in ? range_key<K>(kr[c], rm) : 0xFFFFFFF0u + (unsigned)(i & 1);          // no cell: equal to no neighbour
        s_dirty[i] = 0;
    }
    __syncthreads();
    // ---- 1. heads: thread t scans the cells [5t, 5t + 5); last head at or before i (0: the run began before the window),
    //         first head after i (FIX_W: the run leaves the window)
    {
        const int i0 = FIX_NL * tid;
        bool hd[FIX_NL];
        int lastl = -1, firstl = FIX_W;
#pragma unroll
        for (int c = 0; c < FIX_NL; ++c) {
            const int i = i0 + c;
            hd[c] = i > 0 && s_d[i] != s_d[i - 1];
            if (hd[c]) { lastl = i; if (firstl == FIX_W) firstl = i; }
        }
        int pm = lastl, sm = firstl;                                          // inclusive prefix max / suffix min over the lanes
        for (int o = 1; o < 64; o <<= 1) {
            const int x = __shfl_up(pm, o), y = __shfl_down(sm, o);
            if (lane >= o) pm = x > pm ? x : pm;
            if (lane + o < 64) sm = y < sm ? y : sm;
        }
        if (lane == 63) s_wh[wave] = pm;
        if (lane == 0) s_we[wave] = sm;
        __syncthreads();
        int before = __shfl_up(pm, 1), after = __shfl_down(sm, 1);            // exclusive: heads in earlier / later lanes
        if (lane == 0) before = -1;
        if (lane == 63) after = FIX_W;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before = s_wh[w] > before ? s_wh[w] : before;
            if (w > wave) after = s_we[w] < after ? s_we[w] : after;
        }
        int run_h = before < 0 ? 0 : before;
#pragma unroll
        for (int c = 0; c < FIX_NL; ++c) { if (hd[c]) run_h = i0 + c; s_h[i0 + c] = (unsigned short)run_h; }
        int run_e = after;
#pragma unroll
        for (int c = FIX_NL - 1; c >= 0; --c) { s_e[i0 + c] = (unsigned short)run_e; if (hd[c]) run_e = i0 + c; }
    }
    __syncthreads();
    // ---- 2. inversions mark their run; an owned run longer than FIX_RUN cannot be repaired here
    bool bad = false;
#pragma unroll
    for (int c = 0; c < FIX_NL; ++c) {
        const int i = tid + 256 * c;
        if (i == 0) continue;
        const int h = s_h[i];
        if (h == i) {                                                          // a head
            if (s_d[i] == RANGE_INVALID && i <= FIX_C && w0 + i < n) nvalid[blockIdx.y] = (unsigned)(w0 + i);
            continue;
        }
        if (!(s_k[i] < s_k[i - 1]) || h > FIX_C) continue;                    // no inversion, or the run is the right neighbour's
        if (h < 1) {                                                           // the run began before the window: the left neighbour's, who sees this
            if (i >= FIX_RUN) bad = true;                                      // cell only if the run is short -- and this far in, it is not
            continue;
        }
        if ((int)s_e[i] - h > FIX_RUN) bad = true; else s_dirty[h] = 1;
    }
    if (blockIdx.x == 0 && tid == 0 && s_d[1] == RANGE_INVALID) nvalid[blockIdx.y] = 0u;       // only dropped cells
    if (w0 + FIX_C >= n - 1 && tid == 0) {                                     // the block that holds the last cell: no dropped cell at all
        const int il = (int)(n - 1 - w0);
        if (s_d[il] != RANGE_INVALID) nvalid[blockIdx.y] = (unsigned)n;
    }
    if (__syncthreads_or(bad)) {                                               // the stack goes to the eight-pass path: nothing else to do here
        // (pinned host memory.  A plain system-scope STORE, not a read-modify-write: every writer stores the same 1, and an atomic OR on
        // host memory needs PCIe AtomicOps, which pass-through / virtualised hosts may not route -- round-5 advisor)
        if (tid == 0) __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    // ---- 3. stable rank inside the run; a cell whose place changes writes itself there
#pragma unroll
    for (int c = 0; c < FIX_NL; ++c) {
        const int i = tid + 256 * c;
        const int h = s_h[i];
        if (h < 1 || h > FIX_C || !s_dirty[h] || w0 + i >= n) continue;
        const int e = s_e[i];
        const K k = kr[c];
        int rank = 0;
        for (int j = h; j < e; ++j) { const K kj = s_k[j]; rank += (kj < k) || (kj == k && j < i); }
        if (h + rank != i) { keys[w0 + h + rank] = k; vals[w0 + h + rank] = vr[c]; }
    }
}

// number of valid cells = position of the first dropped cell (key == invalid()) in the sorted keys (one thread:
// a per-wave atomic counter while building the keys serialised 100k atomics on one address = 1.1 ms)
template <typename K>
__global__ void k_count_valid(const K* __restrict__ keys, int64_t n, unsigned* __restrict__ nvalid)
{
    if (threadIdx.x != 0) return;
    keys += (size_t)blockIdx.x * n; nvalid += blockIdx.x;
    int64_t lo = 0, hi = n;                        // first index with keys[idx] == invalid()
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < KeyTraits<K>::invalid()) lo = mid + 1; else hi = mid; }
    *nvalid = (unsigned)lo;
}
