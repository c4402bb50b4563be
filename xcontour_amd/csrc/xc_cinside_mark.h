// The crossing bit planes of K17, shared by K17 (xc_cinside.hip) and K24 (xc_cfold.hip); xc_cinside.hip's header states the rule: bit
// c & 31 of word c >> 5 of row r of a range's plane is X[r][c], ny rows of wpr = ceil(nx / 32) words.  Here: the marks (k_ci_mark), the
// XOR of the rows of every chunk (k_ci_chunk), the cut of the rows into chunks (ci_geometry), the wave sum that closes a column scan, and
// on the host what the two launchers have in common: the blocks of the workspace both keep (CiPlanes) and the step of a group from the
// clearing of its planes to the marks (ci_mark_group).
// Included inside namespace xc { namespace { ... } } after xc_cpiece_select.h and xc_cinside_bound.h; the including file includes <algorithm>.
#pragma once

constexpr int CI_MIN_ROWS = 4;                // a chunk of rows is never shorter (but for the last one) ...
constexpr int CI_MAX_CHUNKS = 64;             // ... and a column is never cut into more chunks
constexpr int64_t CI_BLOCKS = 4096;           // the rows are cut until the scan has about this many blocks

template <typename T>
__device__ __forceinline__ T ci_wave_sum(T v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// a column scan's geometry: a block is CI_TPB columns x rc rows x one range; ncb column blocks, nchunk chunks of rc rows (the last one
// what is left), wpr words per row of a bit plane
struct CiGeom { int64_t wpr, ncb, nchunk, rc; };
inline CiGeom ci_geometry(int64_t ny, int64_t nx, int64_t nrange)
{
    CiGeom g;
    g.wpr = (nx + 31) / 32; g.ncb = (nx + CI_TPB - 1) / CI_TPB;
    int64_t nchunk = (CI_BLOCKS + g.ncb * nrange - 1) / (g.ncb * nrange);
    nchunk = std::min<int64_t>(std::min<int64_t>(nchunk, CI_MAX_CHUNKS), std::max<int64_t>(1, ny / CI_MIN_ROWS));
    g.rc = (ny + nchunk - 1) / nchunk;
    g.nchunk = (ny + g.rc - 1) / g.rc;
    return g;
}

__global__ __launch_bounds__(CP_TPB)
void k_ci_mark(int64_t n, long long s0, int64_t r0, long long E, int64_t nx, int64_t wpr, size_t plane, int select,
               const long long* __restrict__ e_from, const long long* __restrict__ e_to, const int* __restrict__ tab,
               const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ prv, const int* __restrict__ lab,
               const unsigned* __restrict__ pn, const int* __restrict__ pw, const unsigned long long* __restrict__ key,
               unsigned* __restrict__ bits)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int t = root[i], r = rid[i];                                // (k_co_root left 0 <= t < n)
    const bool ring = prv[i] >= 0;
    int w; bool ismain;
    if (!co_selected(select, ring, t, lab[i], pn, pw, key[r0 + r], w, ismain)) return;
    auto cross = [&](long long e) {                                   // 0 <= e < E: the node e >> 1 lies on the plane
        const long long node = e >> 1, row = node / nx, col = node - row * nx;
        atomicOr(bits + (size_t)r * plane + (size_t)row * (size_t)wpr + (size_t)(col >> 5), 1u << (col & 31));
    };
    const long long ef = e_from[s0 + i];
    if ((ef & 1) && ef >= 0 && ef < E) cross(ef);
    if (!ring) {
        const long long et = e_to[s0 + i];
        if ((et & 1) && et >= 0 && et < E) {
            const int j = tab[(size_t)r * E + et];
            if (j < 0 || j >= n) cross(et);                           // no successor: the tail of its piece
        }
    }
}

// cpar[g][chunk][word] = the XOR of the bit plane's words over the rows of the chunk
__global__ __launch_bounds__(CP_TPB)
void k_ci_chunk(int64_t nwords, int64_t ny, int64_t wpr, int64_t rc, int64_t nchunk, const unsigned* __restrict__ bits,
                unsigned* __restrict__ cpar)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= nwords) return;
    const int64_t word = i % wpr, ch = (i / wpr) % nchunk, g = i / (wpr * nchunk);
    const int64_t ra = ch * rc, rb = ra + rc < ny ? ra + rc : ny;
    const unsigned* bp = bits + (size_t)g * (size_t)ny * (size_t)wpr + (size_t)word;
    unsigned x = 0u;
    for (int64_t r = ra; r < rb; ++r) x ^= bp[(size_t)r * (size_t)wpr];
    cpar[i] = x;
}

// The blocks of ctx->cpiece_ws that K17 and K24 both keep, with the scan's geometry: key, nsel [nrange] and mx[nslab][2], the first
// blocks of the run the launcher clears with one fill (its own words follow them), and the planes bits[gmax][ny][wpr],
// cpar[gmax][nchunk][wpr], which stand in front of the tail.  `plane`: the words of one range's bit plane.
struct CiPlanes {
    CiGeom geo; size_t plane;
    unsigned long long* key; int* nsel; unsigned long long* mx; unsigned *bits, *cpar;
    CiPlanes(int64_t ny, int64_t nx, int64_t nrange) : geo(ci_geometry(ny, nx, nrange)), plane((size_t)ny * (size_t)geo.wpr) {}
    void carve_words(Carve& c, int64_t nrange, int64_t nslab)
    {
        key = c.take<unsigned long long>((size_t)nrange); nsel = c.take<int>((size_t)nrange); mx = c.take<unsigned long long>((size_t)nslab * 2);
    }
    void carve_planes(Carve& c, int64_t gmax)
    {
        bits = c.take<unsigned>((size_t)gmax * plane); cpar = c.take<unsigned>((size_t)gmax * (size_t)geo.nchunk * (size_t)geo.wpr);
    }
};

// The step of the group `g` that K17 and K24 share: the group's bit planes cleared (stage 3), phase A up to its rounds, K16's selection
// (stage 2) and the marks.  -> in `s` the roles of the selection.  The launcher goes on behind the k_ci_mark launch: it checks the
// launch (K24 behind its k_cf_rows) and marks stage 3.
inline int ci_mark_group(CpRun& run, const CpGroup& g, const CiPlanes& m, int wrap, int64_t nx, const double* pts, int select, CoRoles& s)
{
    xc_ctx* ctx = run.ctx;
    XC_HIP(ctx, hipMemsetAsync(m.bits, 0, (size_t)(g.r1 - g.r0) * m.plane * 4, ctx->stream));
    run.tm.mark(3);
    run.begin(g);
    XC_TRY(run.rounds());
    s = co_launch_select(run, wrap, nx, pts, select, m.nsel, m.key);
    XC_HIP(ctx, hipGetLastError());
    run.tm.mark(2);
    hipLaunchKernelGGL(k_ci_mark, run.grid, dim3(CP_TPB), 0, ctx->stream, run.n, run.s0, g.r0, run.pl.E, nx, m.geo.wpr, m.plane, select, run.e_from,
                       run.e_to, run.t.tab, run.t.rid, s.root, run.b.prv, run.b.lab, s.pn, s.pw, m.key, m.bits);
    return XC_OK;
}
