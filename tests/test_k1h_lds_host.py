"""K1h on 16x16x32 MFMAs: the LDS layout of the halo and the weight ring, checked on the host.

confild_amd/csrc/k1h_lds.hpp holds the address functions the kernel uses
(conv_x.hip, conv_h16_body) as plain constexpr functions.  tests/k1h_lds_dump.cpp
evaluates them, with the kernel's thread roles, for every lane of every
ds_read_b128 fragment read and every staging store -- every tile width, 9-tap and
phase form, wave row, tap, row block, both channel widths -- and this test applies
the LDS bank model of gfx950 to each wave instruction (the model written down at
lds_swz_bf in unet_kernels.hip):

  ds_read_b128   bank (a / 4) % 64, four lane groups {0-3, 12-15, 20-27},
                 {4-11, 16-19, 28-31} and the same + 32
  ds_write_b64   bank (a / 4) % 32, four groups of 16 consecutive lanes
  ds_write_b128  bank (a / 4) % 32, eight groups of 8 consecutive lanes

Only lanes of one group conflict; the layout must put no two of them on one bank.
The same check must FAIL for the plain (unswizzled) layout's reads, which shows
that it can.  Every offset must also stay inside its plane, a phase-form read
inside the (TR + 1) x (TW + 1) halo that form stages, and no read may touch a
pixel that no thread staged.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "confild_amd", "csrc")
BM = 256

_G0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
_G1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
READ_B128 = [_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1]]
WRITE_B64 = [list(range(16 * k, 16 * k + 16)) for k in range(4)]
WRITE_B128 = [list(range(8 * k, 8 * k + 8)) for k in range(8)]


def hws(tw):
    return (tw + 2 + 7) // 8 * 8


def conflicts(addrs, groups, nbytes, nbanks):
    """extra LDS cycles of one wave instruction: per group, the busiest bank's distinct addresses - 1"""
    extra = 0
    for g in groups:
        per_bank = {}
        for lane in g:
            a = addrs[lane]
            if a < 0:
                continue
            assert a % nbytes == 0, f"misaligned {nbytes}-byte access at {a}"
            for b in range(a // 4, (a + nbytes) // 4):
                per_bank.setdefault(b % nbanks, set()).add(a)
        if per_bank:
            extra += max(len(v) for v in per_bank.values()) - 1
    return extra


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None and os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("k1h") / "k1h_lds_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "k1h_lds_dump.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    recs = {"A": [], "B": [], "S": [], "W": []}
    npar = {"A": 7, "B": 4, "S": 5, "W": 3}
    for line in out.splitlines():
        f = line.split()
        n = npar[f[0]]
        par, addrs = tuple(int(v) for v in f[1:1 + n]), [int(v) for v in f[1 + n:]]
        assert len(addrs) == 64
        recs[f[0]].append((par, addrs))
    return recs


def test_every_instruction_is_enumerated(dump):
    # 2 layouts x 3 tile widths x (9 + 4 taps) x 4 wave rows x 4 row blocks
    assert len(dump["A"]) == 2 * 3 * 13 * 4 * 4
    assert len(dump["B"]) == 2 * (2 + 1) * 4
    assert len(dump["W"]) == 2 * (8 + 4)
    for swz in (0, 1):
        for tw in (64, 32, 16):
            for bn, ntg in ((128, 512), (64, 256)):
                n = sum(1 for p, _ in dump["S"] if p[:3] == (swz, tw, bn))
                assert n == -(-((BM // tw + 2) * (tw + 2) * 8) // ntg) * (ntg // 64)


def test_fragment_reads_conflict_free(dump):
    for tag in ("A", "B"):
        for par, addrs in dump[tag]:
            if par[0] == 1:
                assert conflicts(addrs, READ_B128, 16, 64) == 0, (tag, par)


def test_unswizzled_reads_do_conflict(dump):
    # the negative control: the same check on the plain layout finds conflicts in
    # every fragment read (two lanes of each group on every 16-byte slot they use)
    for tag in ("A", "B"):
        plain = [conflicts(addrs, READ_B128, 16, 64) for par, addrs in dump[tag] if par[0] == 0]
        assert plain and min(plain) > 0, (tag, min(plain))


def test_staging_stores_conflict_free(dump):
    for par, addrs in dump["S"]:
        if par[0] == 1:
            assert conflicts(addrs, WRITE_B64, 8, 32) == 0, ("S", par)
    for par, addrs in dump["W"]:
        if par[0] == 1:
            assert conflicts(addrs, WRITE_B128, 16, 32) == 0, ("W", par)


def test_offsets_stay_inside_their_planes(dump):
    for swz in (0, 1):
        for tw in (64, 32, 16):
            tr = BM // tw
            hplane = (tr + 2) * hws(tw) * 64
            staged = {}   # bn -> LDS (pixel, 8-byte piece) written by the staging stores
            for par, addrs in dump["S"]:
                if par[:2] != (swz, tw):
                    continue
                for a in addrs:
                    if a >= 0:
                        assert 0 <= a and a + 8 <= hplane, ("S", par, a)
                        key = staged.setdefault(par[2], set())
                        assert a not in key, ("S twice", par, a)
                        key.add(a)
            for bn in (128, 64):   # every staged pixel whole: 8 pieces of 8 bytes, and the dense halo only
                px = {a // 64 for a in staged[bn]}
                assert len(staged[bn]) == 8 * len(px) == 8 * (tr + 2) * (tw + 2)
                assert all(p % hws(tw) < tw + 2 and p // hws(tw) < tr + 2 for p in px)
            px = {a // 64 for a in staged[128]}
            for par, addrs in dump["A"]:
                if par[:2] != (swz, tw):
                    continue
                phase = par[2]
                for a in addrs:
                    assert 0 <= a and a + 16 <= hplane, ("A", par, a)
                    p = a // 64
                    row, col = p // hws(tw), p % hws(tw)
                    # the phase form stages (and may read) only (TR + 1) x (TW + 1)
                    assert row < tr + (1 if phase else 2) and col < tw + (1 if phase else 2), ("A", par, a)
                    assert p in px, ("A reads an unstaged pixel", par, a)
    for par, addrs in dump["B"] + dump["W"]:
        bn = par[1]
        for a in addrs:
            assert 0 <= a and a + 16 <= bn * 64, (par, a)
    # the ring's reads cover what the staging stores wrote, nothing else
    for swz in (0, 1):
        for bn in (128, 64):
            w = {a for par, addrs in dump["W"] if par[:2] == (swz, bn) for a in addrs}
            r = {a for par, addrs in dump["B"] if par[:2] == (swz, bn) for a in addrs}
            assert w == r and len(w) == bn * 4
