"""Carve (xcontour_amd/csrc/xc_carve.h), the one statement of a device workspace's layout, without a GPU: a stand-alone program with its
own main, built with the address and undefined-behaviour sanitizers and run as a child process (never loaded into Python), takes a layout
of twelve blocks of mixed element sizes and odd counts through both passes -- measuring and placing -- as the launchers do."""
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
#include "xc_carve.h"
using xc::Carve;

struct Rec24 { double a; unsigned long long b; int c, d; };          // a 24-byte element, like a field record of the ring launchers
static_assert(sizeof(Rec24) == 24, "Rec24");

constexpr int NB = 12;
static const size_t N[NB] = {1, 3, 255, 257, 0, 1, 3, 255, 257, 64, 5, 1000};      // elements
static const size_t ES[NB] = {1, 4, 8, 4, 8, 8, 24, 1, 2, 4, 8, 24};               // bytes of one
struct Lay { void* p[NB]; size_t start[NB]; size_t span; };

// one layout function, run twice; blocks 5, 6 and 7 stand between two marks
static size_t lay(Carve c, Lay& L)
{
#define TAKE(k, T) do { L.start[k] = c.at; L.p[k] = c.take<T>(N[k]); } while (0)
    TAKE(0, unsigned char); TAKE(1, int); TAKE(2, double); TAKE(3, unsigned); TAKE(4, long long);
    const size_t m0 = c.mark();
    TAKE(5, unsigned long long); TAKE(6, Rec24); TAKE(7, unsigned char);
    L.span = c.mark() - m0;
    TAKE(8, short); TAKE(9, int); TAKE(10, double); TAKE(11, Rec24);
#undef TAKE
    return c.at;
}

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); bad = 1; } } while (0)
static size_t padded(int k) { return (N[k] * ES[k] + 255) / 256 * 256; }

int main(void)
{
    static const size_t es_of[NB] = {sizeof(unsigned char), sizeof(int), sizeof(double), sizeof(unsigned), sizeof(long long),
                                     sizeof(unsigned long long), sizeof(Rec24), sizeof(unsigned char), sizeof(short), sizeof(int),
                                     sizeof(double), sizeof(Rec24)};
    for (int k = 0; k < NB; ++k) CHECK(es_of[k] == ES[k]);
    CHECK(xc::al(0) == 0 && xc::al(1) == 256 && xc::al(256) == 256 && xc::al(257) == 512);

    Lay M, P;
    const size_t total = lay(Carve(), M);                                           // measuring: only null pointers
    for (int k = 0; k < NB; ++k) CHECK(M.p[k] == nullptr);
    size_t want = 0;
    for (int k = 0; k < NB; ++k) want += padded(k);
    CHECK(total == want);
    CHECK(M.span == padded(5) + padded(6) + padded(7));                             // two marks around three blocks

    char* base = (char*)malloc(total);                                              // exactly the measured bytes
    CHECK(base != nullptr);
    if (!base) return 1;
    const size_t end = lay(Carve(base), P);                                         // placing
    CHECK(end == total);
    CHECK(P.span == M.span);
    for (int k = 0; k < NB; ++k) {
        CHECK(P.start[k] == M.start[k]);
        CHECK(P.start[k] % 256 == 0);                                               // 256-aligned relative to the base
        CHECK((char*)P.p[k] == base + P.start[k]);
        CHECK((k + 1 < NB ? P.start[k + 1] : end) - P.start[k] == padded(k));
    }
    CHECK(padded(4) == 0 && P.start[5] == P.start[4]);                              // a block of no elements takes no bytes
    // every byte of every block, its padding included: a block that overlaps another or passes the end shows
    for (int k = 0; k < NB; ++k) memset(P.p[k], k + 1, padded(k));
    for (int k = 0; k < NB; ++k)
        for (size_t i = 0; i < padded(k); ++i)
            if (((unsigned char*)P.p[k])[i] != (unsigned char)(k + 1)) { printf("block %d overwritten at byte %zu\n", k, i); bad = 1; break; }
    free(base);
    puts(bad ? "FAILED" : "carve ok");
    return bad;
}
'''


def test_carve_stand_alone_under_sanitizers(tmp_path):
    """both passes of one layout function: the measuring pass returns only null pointers and the bytes the placing pass ends at; every
    block starts 256-aligned and is padded; an empty block takes nothing; two marks give the bytes between them; and a buffer of exactly
    the measured bytes takes a write of every byte of every block under the address sanitizer"""
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')

    def works(cmd):
        return subprocess.run(cmd + ['-o', str(tmp_path / 'probe'), str(probe)], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT).returncode == 0 \
            and subprocess.run([str(tmp_path / 'probe')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0
    # g++ with the runtimes linked into the program itself where the static ones are installed, else with the shared ones, else the
    # clang++ behind hipcc (host code only: -x c++)
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    gxx = shutil.which('g++')
    tries = ([[gxx] + san + ['-static-libasan', '-static-libubsan'], [gxx] + san] if gxx else []) \
        + ([[HIPCC, '-x', 'c++'] + san] if os.path.exists(HIPCC) else [])
    cmd = next((c for c in tries if works(c)), None)
    if cmd is None:
        pytest.skip('no compiler with a sanitizer runtime')
    main = tmp_path / 'carve_main.cpp'
    main.write_text(MAIN)
    exe = str(tmp_path / 'carve_main')
    subprocess.run(cmd + ['-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-I', CSRC, '-o', exe, str(main)], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and 'carve ok' in r.stdout, r.stdout
