// The crossing bit planes of K17, shared by K17 (xc_cinside.hip) and K24 (xc_cfold.hip); xc_cinside.hip's header states the rule: bit
// c & 31 of word c >> 5 of row r of a range's plane is X[r][c], ny rows of wpr = ceil(nx / 32) words.  Here: the marks (k_ci_mark), the
// XOR of the rows of every chunk (k_ci_chunk), the cut of the rows into chunks (ci_geometry) and the wave sum that closes a column scan.
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
