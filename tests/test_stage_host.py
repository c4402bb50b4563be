"""Stage and lay_stage (xcontour_amd/csrc/xc_stage.h), the one statement of a host form's arena layout, without a GPU: a stand-alone
program with its own main, built with the address and undefined-behaviour sanitizers and run as a child process (never loaded into
Python), runs one layout function -- inputs, an optional input, four optional results of every kind -- through lay_stage for every
combination of null and non-null optional arguments, with the pinned buffer granting and refusing direct results.  The three functions
of the library that the header declares are stand-ins here: an arena of exactly the measured bytes, a pinned buffer, a log of d2h."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'xcontour_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')

MAIN = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "xc_stage.h"
using xc::Stage;

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d (case %d, direct %zu): %s\n", __LINE__, g_case, g_direct, #cond); bad = 1; } } while (0)
static int g_case = 0; static size_t g_direct = 0;

struct xc_ctx {
    char* arena = nullptr; size_t arena_bytes = 0, asked = 0; int grows = 0;
    char pin[1024]; size_t pin_off = 0, direct_max = 0; int direct_calls = 0;
    struct Copy { void* h; const void* d; size_t n; } copies[16]; int ncopy = 0;
};
namespace xc {
int ensure_arena(xc_ctx* ctx, size_t bytes, void** base)                    // exactly the bytes asked for: one byte past them is the sanitizer's
{
    ++ctx->grows; ctx->asked = bytes;
    free(ctx->arena); ctx->arena = (char*)malloc(bytes ? bytes : 1); ctx->arena_bytes = bytes;
    *base = ctx->arena;
    return ctx->arena ? 0 : -4;
}
void* out_direct(xc_ctx* ctx, void* h, size_t n)
{
    ++ctx->direct_calls;
    if (!h || n == 0 || n > ctx->direct_max || ctx->pin_off + n > sizeof(ctx->pin)) return nullptr;
    char* p = ctx->pin + ctx->pin_off; ctx->pin_off += (n + 63) & ~(size_t)63;
    return p;
}
int d2h(xc_ctx* ctx, void* h, const void* d, size_t n) { ctx->copies[ctx->ncopy++] = {h, d, n}; memcpy(h, d, n); return 0; }
}

// the blocks of the layout: 0 q, 1 coordinates, 2 levels (optional input), 3 nothing (no bytes), 4 A out(), 5 B out(direct), 6 C keep(), 7 D keep(direct)
constexpr int NB = 8;
static const size_t BYTES[NB] = {1000, 56, 280, 0, 280, 56, 8, 300};
struct Ptrs { void* p[NB]; size_t start[NB]; bool took[NB]; };
struct Args { const double* levels; double *A, *B, *C, *D; };

static void lay(Stage& s, const Args& a, Ptrs& P)
{
    for (int k = 0; k < NB; ++k) { P.p[k] = nullptr; P.start[k] = 0; P.took[k] = false; }
#define AT(k) do { P.start[k] = s.c.at; P.took[k] = true; } while (0)
    AT(0); P.p[0] = s.take(BYTES[0]);
    AT(1); P.p[1] = s.take<double>(BYTES[1]);
    if (a.levels) { AT(2); P.p[2] = s.take<double>(BYTES[2]); }
    AT(3); P.p[3] = s.take(BYTES[3]);
    AT(4); P.p[4] = s.out(a.A, BYTES[4]);
    AT(5); P.p[5] = s.out(a.B, BYTES[5], true);
    AT(6); P.p[6] = s.keep(a.C, BYTES[6]);
    AT(7); P.p[7] = s.keep(a.D, BYTES[7], true);
#undef AT
}

static bool in_pin(const xc_ctx& c, const void* p) { return (const char*)p >= c.pin && (const char*)p < c.pin + sizeof(c.pin); }

int main(void)
{
    static double levels[35], A[35], B[7], C[1], D[38];
    for (g_direct = 0; g_direct <= 512; g_direct += 256)                            // the pinned buffer grants nothing / B only / B and D
        for (g_case = 0; g_case < 32; ++g_case) {
            const Args a = {g_case & 1 ? levels : nullptr, g_case & 2 ? A : nullptr, g_case & 4 ? B : nullptr, g_case & 8 ? C : nullptr,
                            g_case & 16 ? D : nullptr};
            xc_ctx ctx; ctx.direct_max = g_direct;
            // measuring alone: null pointers, no pinned bytes, no hand-over, nothing owed
            Ptrs M; Stage m(&ctx); lay(m, a, M);
            for (int k = 0; k < NB; ++k) CHECK(M.p[k] == nullptr);
            CHECK(m.nout == 0 && ctx.direct_calls == 0 && ctx.pin_off == 0 && ctx.grows == 0 && ctx.ncopy == 0);
            size_t want = 0;                                                        // what today's rule counts: every block but a null out()
            const bool present[NB] = {true, true, a.levels != nullptr, true, a.A != nullptr, a.B != nullptr, true, true};
            for (int k = 0; k < NB; ++k) if (present[k]) want += xc::al(BYTES[k]);
            CHECK(m.c.at == want);
            // the helper: measured, the arena grown once to that, placed
            Ptrs P; Stage st(&ctx);
            CHECK(xc::lay_stage(st, [&](Stage& s) { lay(s, a, P); }) == 0);
            CHECK(ctx.grows == 1 && ctx.asked == want && st.c.base == ctx.arena);
            CHECK(st.c.at <= want);                                                 // the measured total is never below the placed one
            const bool dB = a.B && BYTES[5] <= g_direct, dD = a.D && BYTES[7] <= g_direct;
            CHECK(ctx.direct_calls == (a.B ? 1 : 0) + (a.D ? 1 : 0));               // once per result that may go direct, placing only
            CHECK(st.c.at == want - (dB ? xc::al(BYTES[5]) : 0) - (dD ? xc::al(BYTES[7]) : 0));
            size_t shift = 0;
            for (int k = 0; k < NB; ++k) {
                CHECK(P.took[k] == M.took[k]);
                if (!P.took[k]) continue;
                CHECK(P.start[k] == M.start[k] - shift);                            // the placed offsets are the measured ones, less what went direct
                const bool direct = (k == 5 && dB) || (k == 7 && dD);
                if (direct) { CHECK(in_pin(ctx, P.p[k])); shift += xc::al(BYTES[k]); }
                else if (present[k]) { CHECK((char*)P.p[k] == ctx.arena + P.start[k]); memset(P.p[k], k + 1, xc::al(BYTES[k])); }
                else CHECK(P.p[k] == nullptr);
            }
            if (g_direct == 0) for (int k = 0; k < NB; ++k) CHECK(P.start[k] == M.start[k]);
            for (int k = 0; k < NB; ++k)                                              // no block overlaps another
                if (present[k] && P.p[k] && !in_pin(ctx, P.p[k]))
                    for (size_t i = 0; i < xc::al(BYTES[k]); ++i) if (((unsigned char*)P.p[k])[i] != k + 1) { CHECK(!"overwritten"); break; }
            // outs[]: only the non-null results that stayed in the arena, in the order they were asked for; deliver() copies in that order
            const void* hosts[4]; const void* devs[4]; size_t bytes[4]; int n = 0;
            if (a.A) { hosts[n] = a.A; devs[n] = P.p[4]; bytes[n++] = BYTES[4]; }
            if (a.B && !dB) { hosts[n] = a.B; devs[n] = P.p[5]; bytes[n++] = BYTES[5]; }
            if (a.C) { hosts[n] = a.C; devs[n] = P.p[6]; bytes[n++] = BYTES[6]; }
            if (a.D && !dD) { hosts[n] = a.D; devs[n] = P.p[7]; bytes[n++] = BYTES[7]; }
            CHECK(st.nout == n);
            for (int i = 0; i < n && i < st.nout; ++i) CHECK(st.outs[i].host == hosts[i] && st.outs[i].dev == devs[i] && st.outs[i].bytes == bytes[i]);
            CHECK(st.deliver() == 0 && ctx.ncopy == n);
            for (int i = 0; i < n && i < ctx.ncopy; ++i) CHECK(ctx.copies[i].h == hosts[i] && ctx.copies[i].d == devs[i] && ctx.copies[i].n == bytes[i]);
            free(ctx.arena);
        }
    puts(bad ? "FAILED" : "stage ok");
    return bad;
}
'''


def test_stage_stand_alone_under_sanitizers(tmp_path):
    """lay_stage over one layout for all 32 combinations of null optional arguments and three sizes of the direct path: measuring forms no
    pointer, calls out_direct never and owes nothing; the arena is grown once to the measured bytes, which are today's sum without the
    null outputs; the placed offsets are the measured ones (less the results that went to the pinned buffer, which measuring counted: the
    measured total is never below the placed one); out_direct is called once per result, placing only; outs[] and deliver() hold the
    non-null arena-backed results in order; and an arena of exactly the measured bytes takes a write of every byte of every block"""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')

    def works(cmd):
        return subprocess.run(cmd + ['-o', str(tmp_path / 'probe'), str(probe)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT).returncode == 0 \
            and subprocess.run([str(tmp_path / 'probe')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0
    # (the compilers of tests/test_carve_host.py, in its order)
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    gxx = shutil.which('g++')
    tries = ([[gxx] + san + ['-static-libasan', '-static-libubsan'], [gxx] + san] if gxx else []) \
        + ([[HIPCC, '-x', 'c++'] + san] if os.path.exists(HIPCC) else [])
    cmd = next((c for c in tries if works(c)), None)
    if cmd is None:
        pytest.skip('no compiler with a sanitizer runtime')
    main = tmp_path / 'stage_main.cpp'
    main.write_text(MAIN)
    exe = str(tmp_path / 'stage_main')
    subprocess.run(cmd + ['-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-I', CSRC, '-o', exe, str(main)], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and 'stage ok' in r.stdout, r.stdout
