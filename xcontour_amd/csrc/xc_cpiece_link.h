// Phase A of the device joins, shared by K13 (xc_cpiece.hip), K14 (xc_cjoin.hip), K16 (xc_coverturn.hip), K17 (xc_cinside.hip),
// K18-K21 (xc_cprecords.hip) and K24 (xc_cfold.hip): the dense edge tables of a GROUP of consecutive ranges, the next / prev links, the pointer-doubling rounds,
// and the host frame every one of these launchers runs them in.  xc_cpiece.hip's header states the rule.  Written once here: the plan
// (cp_plan: counts, scan, the refusal of segments without records, groups), the tail of the workspace (cp_carve_tail), the per-group
// run (CpRun: offsets up, table filled, then begin / rounds / end per group with their stage marks and the sum of the rounds) and the
// read of the error word (cp_read_err).  What stays with a launcher: the head of its workspace, its own stages between rounds() and
// end(), the meaning of the error bits, and whether it returns on a call without segments (K13, K14, K18-K21) or goes on with an empty
// plan (K16, K17, K24).  Included inside namespace xc { namespace { ... } } after xc_capi.h, like xc_binning.h.
#pragma once

constexpr int CP_TPB = 256;
constexpr int CP_ERR_EDGE = 1, CP_ERR_LINK = 2;
constexpr size_t CP_SMALL = 64;               // the ints of the block that holds a call's error word (and K13's c0): 256 bytes

// largest r in [lo, hi) with off[r] <= i (off ascending, off[lo] <= i < off[hi])
__device__ __forceinline__ int64_t cp_range_of(const long long* __restrict__ off, int64_t lo, int64_t hi, long long i)
{
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(CP_TPB)
void k_cp_scatter(int64_t n, long long s0, const long long* __restrict__ off, int64_t r0, int64_t r1, long long E,
                  const long long* __restrict__ e_from, int* __restrict__ tab, int* __restrict__ rid, int* __restrict__ lab,
                  int* __restrict__ prv, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int rl = (int)(cp_range_of(off, r0, r1, s0 + i) - r0);
    const long long e = e_from[s0 + i];
    rid[i] = rl;
    prv[i] = -1;
    if (e < 0 || e >= E) { lab[i] = 0x7fffffff; *err = CP_ERR_EDGE; return; }
    lab[i] = (int)e;
    tab[(size_t)rl * E + e] = (int)i;
}

__global__ __launch_bounds__(CP_TPB)
void k_cp_link(int64_t n, long long s0, long long E, const long long* __restrict__ e_to, const int* __restrict__ tab,
               const int* __restrict__ rid, int* __restrict__ nxt, int* __restrict__ prv, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const long long e = e_to[s0 + i];
    int j = -1;
    if (e < 0 || e >= E) *err = CP_ERR_EDGE;
    else j = tab[(size_t)rid[i] * E + e];
    if (j >= n) j = -1;
    nxt[i] = j;
    if (j >= 0) prv[j] = (int)i;
}

__global__ __launch_bounds__(CP_TPB)
void k_cp_round(int64_t n, const int* __restrict__ lab, const int* __restrict__ nxt, const int* __restrict__ prv,
                int* __restrict__ lab2, int* __restrict__ nxt2, int* __restrict__ prv2)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int a = nxt[i], b = prv[i];
    int l = lab[i], a2 = -1, b2 = -1;
    if (a >= 0) { const int la = lab[a]; l = la < l ? la : l; a2 = nxt[a]; }
    if (b >= 0) { const int lb = lab[b]; l = lb < l ? lb : l; b2 = prv[b]; }
    lab2[i] = l; nxt2[i] = a2; prv2[i] = b2;
}

__global__ __launch_bounds__(CP_TPB)
void k_cp_unscatter(int64_t n, long long s0, long long E, const long long* __restrict__ e_from, const int* __restrict__ rid,
                    int* __restrict__ tab)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const long long e = e_from[s0 + i];
    if (e >= 0 && e < E) tab[(size_t)rid[i] * E + e] = -1;
}

inline unsigned cp_blocks(int64_t n) { return (unsigned)((n + CP_TPB - 1) / CP_TPB); }

// groups of consecutive ranges [r0, r1): the table rows fit the cap (one range always does), fewer than 2^31 segments; empty ranges in
// front of a group or behind it cost no table row.  hc: the counts, off: their exclusive scan.  gmax / nmax: the most rows / segments
// of one group.
struct CpGroup { int64_t r0, r1; };
inline std::vector<CpGroup> cp_plan_groups(size_t cap, long long E, int64_t nrange, const std::vector<uint64_t>& hc,
                                           const std::vector<long long>& off, int64_t* gmax, long long* nmax)
{
    std::vector<CpGroup> groups;
    *gmax = 1; *nmax = 0;
    int64_t rows_cap = (int64_t)(cap / ((size_t)E * 4));
    if (rows_cap < 1) rows_cap = 1;
    int64_t r = 0;
    while (r < nrange) {
        while (r < nrange && hc[(size_t)r] == 0) ++r;
        if (r >= nrange) break;
        int64_t r1 = r + 1;
        while (r1 < nrange && r1 - r < rows_cap && off[(size_t)r1 + 1] - off[(size_t)r] < (1ll << 31) - 1) ++r1;
        while (r1 - 1 > r && hc[(size_t)r1 - 1] == 0) --r1;
        groups.push_back({r, r1});
        if (r1 - r > *gmax) *gmax = r1 - r;
        if (off[(size_t)r1] - off[(size_t)r] > *nmax) *nmax = off[(size_t)r1] - off[(size_t)r];
        r = r1;
    }
    return groups;
}

// the doubling rounds of a group: ceil(log2(its largest count)) + 1, from the host's counts
inline int cp_rounds(const std::vector<uint64_t>& hc, const CpGroup& g)
{
    uint64_t cmaxg = 1;
    for (int64_t r = g.r0; r < g.r1; ++r) if (hc[(size_t)r] > cmaxg) cmaxg = hc[(size_t)r];
    int R = 1;
    while ((1ull << (R - 1)) < cmaxg) ++R;
    return R;
}

// K12's counts on the host and their exclusive scan: one wait for the stream.  `clear` (the call's own per-range counts, or null) is
// cleared between the copy and the wait.
inline int cp_read_counts(xc_ctx* ctx, const char* who, int64_t nrange, const uint64_t* count, uint64_t* clear, std::vector<uint64_t>& hc,
                          std::vector<long long>& off)
{
    hc.resize((size_t)nrange);
    XC_HIP(ctx, hipMemcpyAsync(hc.data(), count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (clear) XC_HIP(ctx, hipMemsetAsync(clear, 0, (size_t)nrange * 8, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    off.assign((size_t)nrange + 1, 0);
    for (int64_t r = 0; r < nrange; ++r) {
        if (hc[(size_t)r] >= (1ull << 31)) return fail(ctx, XC_EBADARG, std::string(who) + ": a range of 2^31 or more segments");
        off[(size_t)r + 1] = off[(size_t)r] + (long long)hc[(size_t)r];
    }
    return XC_OK;
}

// The plan of a call: the counts, their scan, and the groups.  A call without segments has no group, no table row (gmax 0) and no
// buffer (nmax 0): K13, K14 and K18-K21 return on total == 0, K16, K17 and K24 go on and write their dense outputs.
struct CpPlan {
    std::vector<uint64_t> hc; std::vector<long long> off; long long total = 0, E = 0;
    std::vector<CpGroup> groups; int64_t gmax = 0; long long nmax = 0;
};
// `who`: the entry, for the refusals; `clear` as for cp_read_counts; one wait for the stream
inline int cp_plan(xc_ctx* ctx, const char* who, int64_t nrange, const uint64_t* count, uint64_t* clear, const int64_t* e_from,
                   const int64_t* e_to, const double* pts, long long E, CpPlan& p)
{
    XC_TRY(cp_read_counts(ctx, who, nrange, count, clear, p.hc, p.off));
    p.total = p.off[(size_t)nrange]; p.E = E;
    if (p.total == 0) return XC_OK;
    if (!e_from || !e_to || !pts) return fail(ctx, XC_EBADARG, std::string(who) + ": segments without their records");
    p.groups = cp_plan_groups(ctx->cpiece_cap, E, nrange, p.hc, p.off, &p.gmax, &p.nmax);
    return XC_OK;
}

// The tail of every layout of ctx->cpiece_ws that runs phase A: tab[gmax][E] | rid[nmax] | nbuf buffers [nmax] (six: label, next,
// prev x 2; K14 ten), taken from the launcher's carve (xc_carve.h).  What lies in front of it is the launcher's own.
constexpr int CP_NBUF = 10;
struct CpTail { int *tab, *rid, *buf[CP_NBUF]; };
inline void cp_carve_tail(Carve& c, const CpPlan& pl, int nbuf, CpTail& t)
{
    t.tab = c.take<int>((size_t)pl.gmax * (size_t)pl.E);
    t.rid = c.take<int>((size_t)pl.nmax);
    for (int k = 0; k < nbuf; ++k) t.buf[k] = c.take<int>((size_t)pl.nmax);
}

// the error word of a call on the host: one wait for the stream.  What its bits mean is the entry's.
inline int cp_read_err(xc_ctx* ctx, const int* d_err, int* herr)
{
    XC_HIP(ctx, hipMemcpyAsync(herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return XC_OK;
}

// which of a group's six buffers [nmax] hold what: lab, nxt and prv stand, lab2, nxt2 and prv2 are free
struct CpRoles { int *lab, *nxt, *prv, *lab2, *nxt2, *prv2; };

// Phase A of one call, group by group.  A launcher's loop is
//     for (const CpGroup& g : plan.groups) { run.begin(g); [K14: its checks] XC_TRY(run.rounds()); its own stages; XC_TRY(run.end()); }
// between upload_off() / fill_table() in front (nothing without groups) and report() behind.  Stage 0 takes the table (and whatever the
// launcher put behind it), stage 1 the rounds, stage 0 again the unscatter; what lies between rounds() and end() the launcher marks.
struct CpRun {
    xc_ctx* ctx; StageTimer& tm; const CpPlan& pl; const long long *e_from, *e_to; long long* d_off; CpTail t; int* d_err;
    // the group at hand: its first segment, its segments, its rounds, its grid of CP_TPB threads, the roles of its buffers
    CpGroup g = {0, 0}; long long s0 = 0; int64_t n = 0; int R = 0; dim3 grid; CpRoles b = {};
    int rounds_total = 0;

    CpRun(xc_ctx* c, StageTimer& timer, const CpPlan& plan, const int64_t* ef, const int64_t* et, long long* off, const CpTail& tail, int* err)
        : ctx(c), tm(timer), pl(plan), e_from((const long long*)ef), e_to((const long long*)et), d_off(off), t(tail), d_err(err) {}
    int upload_off()
    {
        if (pl.groups.empty()) return XC_OK;
        XC_HIP(ctx, hipMemcpyAsync(d_off, pl.off.data(), pl.off.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        return XC_OK;
    }
    int fill_table()
    {
        if (pl.groups.empty()) return XC_OK;
        XC_HIP(ctx, hipMemsetAsync(t.tab, 0xff, (size_t)pl.gmax * (size_t)pl.E * 4, ctx->stream));
        return XC_OK;
    }
    // the edge table of the group and the links
    void begin(const CpGroup& group)
    {
        g = group; s0 = pl.off[(size_t)g.r0]; n = pl.off[(size_t)g.r1] - s0; R = cp_rounds(pl.hc, g); grid = dim3(cp_blocks(n));
        b = {t.buf[0], t.buf[1], t.buf[2], t.buf[3], t.buf[4], t.buf[5]};
        hipLaunchKernelGGL(k_cp_scatter, grid, dim3(CP_TPB), 0, ctx->stream, n, s0, d_off, g.r0, g.r1, pl.E, e_from, t.tab, t.rid, b.lab, b.prv, d_err);
        hipLaunchKernelGGL(k_cp_link, grid, dim3(CP_TPB), 0, ctx->stream, n, s0, pl.E, e_to, t.tab, t.rid, b.nxt, b.prv, d_err);
    }
    // R doubling rounds: b holds the roles after them
    int rounds()
    {
        XC_HIP(ctx, hipGetLastError());
        tm.mark(0);
        for (int k = 0; k < R; ++k) {
            hipLaunchKernelGGL(k_cp_round, grid, dim3(CP_TPB), 0, ctx->stream, n, b.lab, b.nxt, b.prv, b.lab2, b.nxt2, b.prv2);
            std::swap(b.lab, b.lab2); std::swap(b.nxt, b.nxt2); std::swap(b.prv, b.prv2);
        }
        XC_HIP(ctx, hipGetLastError());
        rounds_total += R;
        tm.mark(1);
        return XC_OK;
    }
    // the table handed on clean
    int end()
    {
        hipLaunchKernelGGL(k_cp_unscatter, grid, dim3(CP_TPB), 0, ctx->stream, n, s0, pl.E, e_from, t.rid, t.tab);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(0);
        return XC_OK;
    }
    void report(CpProfile& p) const { p.rounds = rounds_total; p.groups = (int)pl.groups.size(); }
};

// The row chunks of a column scan (K20, K21: xc_cpiece_label.h; K22: xc_cpoverlap.hip).
constexpr int PL_ROWS = 16;                   // a chunk of a column has at least this many rows ...
constexpr int PL_CHUNKS = 32;                 // ... and a column at most this many chunks

// the chunks of a column: `rows` rows each (the last one what is left), `nchunk` of them
inline void pl_geometry(int64_t ny, int64_t* rows, int64_t* nchunk)
{
    int64_t R = (ny + PL_CHUNKS - 1) / PL_CHUNKS;
    if (R < PL_ROWS) R = PL_ROWS;
    *rows = R; *nchunk = (ny + R - 1) / R;
}

// thread -> (range of the group, chunk, column), columns fastest
__device__ __forceinline__ bool pl_thread(int64_t ng, int64_t nchunk, int64_t nx, int64_t& rl, int64_t& k, int64_t& c)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= ng * nchunk * nx) return false;
    const int64_t rk = i / nx;
    c = i - rk * nx; rl = rk / nchunk; k = rk - rl * nchunk;
    return true;
}
