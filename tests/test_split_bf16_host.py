"""split_bf16.h on the host: a stand-alone program (its own main) includes
the header, splits a fixed set of floats and checks every one itself:

* each piece has its low 16 bits clear (it is a bf16 value),
* (double)hi + mid + lo == (double)v exactly, for every normal input,
* no piece is non-finite,
* denormal inputs (whose lo can keep bits below the bf16 range): only that
  the pieces are finite and sum to within one fp32 denormal step of v.

The low-16-bits check is skipped for a piece that is itself below the normal
range (|piece| < 2^-126; this happens to mid or lo of normal inputs below
2^-110, whose last significant bit lies under 2^-133): a bf16 value there is
a multiple of 2^-133, so a sum of such pieces cannot equal an input that is
not one.  The exact-sum check still applies to those inputs, and the kernel
drops at most 2^-133 of them when it takes the upper half of the word.

Inputs: +-0, the smallest and largest normal floats, 1 +- 1 ulp, every power
of two of the normal range, and 1e5 pseudo-random floats (xorshift bit
patterns) over the whole normal exponent range, both signs.
"""
import os
import shutil
import subprocess

import pytest

HDR_DIR = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    "distributedkernelshap_amd", "ops", "hip",
)

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "split_bf16.h"

static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static long n_checked = 0, n_denormal = 0;

static int check(float v) {
    const SplitBf16 s = split_bf16(v);
    const float piece[3] = {s.hi, s.mid, s.lo};
    const bool denormal = v != 0.0f && std::fabs(v) < 1.17549435e-38f;
    ++n_checked;
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(piece[i])) {
            printf("FAIL non-finite piece %d of %a\n", i, v); return 1;
        }
        // a piece below the normal range has a resolution of 2^-149 in fp32
        // but 2^-133 in bf16: no split can keep both the exact sum and clear
        // low bits there (see the module docstring)
        const bool tiny = std::fabs(piece[i]) < 1.17549435e-38f;
        if (denormal || tiny) continue;
        if (bits(piece[i]) & 0xFFFFu) {
            printf("FAIL low bits set in piece %d of %a\n", i, v); return 1;
        }
        if (split_bf16_pattern(piece[i]) != (uint16_t)(bits(piece[i]) >> 16)) {
            printf("FAIL pattern of piece %d of %a\n", i, v); return 1;
        }
    }
    const double sum = (double)s.hi + (double)s.mid + (double)s.lo;
    if (denormal) {
        ++n_denormal;
        // one fp32 denormal step = 2^-149
        if (std::fabs(sum - (double)v) > std::ldexp(1.0, -149)) {
            printf("FAIL denormal %a: sum %a\n", v, sum); return 1;
        }
    } else if (sum != (double)v) {
        printf("FAIL %a: hi %a mid %a lo %a sum %a\n", v, s.hi, s.mid, s.lo, sum);
        return 1;
    }
    return 0;
}

int main() {
    int bad = 0;
    bad |= check(0.0f);
    bad |= check(-0.0f);
    const float fmin_n = from_bits(0x00800000u), fmax_n = from_bits(0x7F7FFFFFu);
    bad |= check(fmin_n); bad |= check(-fmin_n);
    bad |= check(fmax_n); bad |= check(-fmax_n);
    bad |= check(from_bits(0x3F800001u)); bad |= check(from_bits(0x3F7FFFFFu));
    bad |= check(-from_bits(0x3F800001u)); bad |= check(-from_bits(0x3F7FFFFFu));
    for (int e = -126; e <= 127; ++e) {
        bad |= check(std::ldexp(1.0f, e));
        bad |= check(-std::ldexp(1.0f, e));
    }
    // denormals: smallest, largest, a few in between
    bad |= check(from_bits(0x00000001u)); bad |= check(from_bits(0x007FFFFFu));
    bad |= check(from_bits(0x80000001u)); bad |= check(from_bits(0x00012345u));
    bad |= check(from_bits(0x80654321u));
    // 1e5 pseudo-random normal floats: exponent field 1..254, both signs
    uint32_t x = 2463534242u;
    for (int i = 0; i < 100000; ++i) {
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        uint32_t y = x;
        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
        const uint32_t expo = 1u + (y >> 8) % 254u;
        const uint32_t u = (x & 0x807FFFFFu) | (expo << 23);
        bad |= check(from_bits(u));
        if (bad) break;
    }
    printf("checked %ld values (%ld denormal): %s\n", n_checked, n_denormal,
           bad ? "FAIL" : "OK");
    return bad;
}
"""


def _compiler():
    for cc in ("g++", "c++", "clang++"):
        path = shutil.which(cc)
        if path:
            return [path]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++"]   # host-only: plain C++, no device pass
    return None


def test_split_bf16_is_exact_on_the_host(tmp_path):
    cc = _compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "split_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "split_main"
    subprocess.run(
        cc + ["-O2", "-std=c++17", "-I", HDR_DIR, str(src), "-o", str(exe)],
        check=True,
    )
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "checked 100523 values (5 denormal): OK" in res.stdout
