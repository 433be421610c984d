"""The host merge of the per-event cluster report (ksim_report_merge, csrc/ksim_report_host.hpp): no GPU.

The shards of a node-sharded cluster each hold the exact record of their own nodes (ksim_report_part: 9 signed 128-bit
sums with LSB 2^-80 and 8 counters); the cluster's report is their integer sum, each 128-bit sum rounded to a double
once.  Here seeded random records are merged twice -- by the stand-alone program tests/native_report (the header under
the address and undefined-behaviour sanitizers) and by the library's ksim_report_merge through ctypes, loaded without
a device -- and compared with Python's big-integer sums, float(Fraction(total, 2**80)) being the correctly rounded
value.  The cases hold low halves whose sum carries past 2^64, a part that is all zero, sums that lie exactly between
two doubles, negative terms, and one case where rounding every part first gives another bin than the exact merge.
"""
import ctypes as C
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

import ksim

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native_report")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 80
PER_WORLD = 125  # x 16 worlds = 2000 merged records


def set_part(p, fx, cnt):
    for k, v in enumerate(fx):
        u = v & ((1 << 128) - 1)
        lo, hi = u & ((1 << 64) - 1), u >> 64
        p.fx[k][0] = lo - (1 << 64) if lo >> 63 else lo
        p.fx[k][1] = hi - (1 << 64) if hi >> 63 else hi
    for k, v in enumerate(cnt):
        p.cnt[k] = v


def split(rnd, total, world, lo_heavy=False):
    """`world` signed terms adding up to total; lo_heavy: low halves near 2^64 (their sum carries)."""
    terms = []
    for _ in range(world - 1):
        t = rnd.randrange(-abs(total) - ONE, abs(total) + ONE)
        if lo_heavy:
            t = (t >> 64 << 64) | ((1 << 64) - 1 - rnd.randrange(1 << 20))
        terms.append(t)
    terms.append(total - sum(terms))
    return terms


def tie(rnd):
    """A value (in units of 2^-80) exactly between two doubles: a 54-bit odd mantissa."""
    m = (1 << 53) | (rnd.getrandbits(52) << 1) | 1
    return m << rnd.randrange(0, 60)


def make_record(rnd, world, kind):
    """-> (per-shard (fx[9], cnt[8]) list, total fx[9], total cnt[8])"""
    fx_tot, shard_fx = [], [[] for _ in range(world)]
    for k in range(9):
        if kind == "tie":
            total = tie(rnd)
        elif kind == "small":
            total = rnd.randrange(0, 1 << 70)
        else:
            total = rnd.randrange(-(1 << 110), 1 << 118)
        terms = split(rnd, total, world, lo_heavy=(kind == "carry"))
        fx_tot.append(total)
        for s in range(world):
            shard_fx[s].append(terms[s])
    cnt_tot, shard_cnt = [], [[] for _ in range(world)]
    for k in range(8):
        terms = [rnd.randrange(-(1 << 40), 1 << 58) for _ in range(world)]
        cnt_tot.append(sum(terms))
        for s in range(world):
            shard_cnt[s].append(terms[s])
    if kind == "zero":  # one shard holds nothing (no node of its own changed, rank > 0): its term moves to another
        z = rnd.randrange(world)
        o = (z + 1) % world
        if o != z:
            for k in range(9):
                shard_fx[o][k] += shard_fx[z][k]
                shard_fx[z][k] = 0
            for k in range(8):
                shard_cnt[o][k] += shard_cnt[z][k]
                shard_cnt[z][k] = 0
    return [(shard_fx[s], shard_cnt[s]) for s in range(world)], fx_tot, cnt_tot


def expected(fx_tot, cnt_tot):
    bins = [float(Fraction(v, ONE)) for v in fx_tot]
    rep = dict(frag_bins=bins[:7], used_nodes=cnt_tot[0], used_gpus=cnt_tot[1], used_gpu_milli=cnt_tot[2],
               total_gpus=cnt_tot[7], arrived_gpu_milli=cnt_tot[4], used_cpu_milli=cnt_tot[3],
               arrived_cpu_milli=cnt_tot[5])
    pw = dict(cluster_w=bins[7] + bins[8], cpu_w=bins[7], gpu_w=bins[8], invalid_nodes=cnt_tot[6])
    return rep, pw


@pytest.fixture(scope="module")
def cases():
    """[(world, [ReportPart array per shard], [expected (report, power)])], 2000 records over worlds 1..16"""
    rnd = random.Random(20240807)
    kinds = ["carry", "zero", "tie", "small", "any"]
    out = []
    for world in range(1, 17):
        arrs = [(ksim.ReportPart * PER_WORLD)() for _ in range(world)]
        want = []
        for i in range(PER_WORLD):
            shards, fx_tot, cnt_tot = make_record(rnd, world, kinds[i % len(kinds)])
            for s in range(world):
                set_part(arrs[s][i], *shards[s])
            want.append(expected(fx_tot, cnt_tot))
        out.append((world, arrs, want))
    return out


def exactness_case():
    """Three shards each holding 1 + 2^-53 in bin 0: every part rounds to 1.0 (a tie, to even), so the sum of the
    rounded parts is 3.0, while the exact sum 3 + 3 * 2^-53 rounds to 3 + 2^-51."""
    arrs = [(ksim.ReportPart * 1)() for _ in range(3)]
    for a in arrs:
        set_part(a[0], [ONE + (1 << 27)] + [0] * 8, [0] * 8)
    naive = sum(float(Fraction(ONE + (1 << 27), ONE)) for _ in range(3))
    exact = float(Fraction(3 * (ONE + (1 << 27)), ONE))
    assert naive == 3.0 and exact == 3.0 + 2.0 ** -51 and naive != exact
    return arrs, exact


def lib_merge(arrs):
    return ksim.report_merge(arrs)


def test_struct_size():
    assert C.sizeof(ksim.ReportPart) == 208  # (the C side: a static_assert of the header and of the check program)


def test_library_merges_without_a_device(cases):
    # the library loads and ksim_report_merge runs with no device: host arithmetic only
    n_rec = 0
    for world, arrs, want in cases:
        reports, power = lib_merge(arrs)
        assert len(reports) == PER_WORLD
        for i, (wr, wp) in enumerate(want):
            assert reports[i] == wr, (world, i)
            assert power[i] == wp, (world, i)
        n_rec += len(reports)
    assert n_rec == 2000


def test_library_merge_is_exact_where_rounded_parts_are_not():
    arrs, exact = exactness_case()
    reports, _ = lib_merge(arrs)
    assert reports[0]["frag_bins"][0] == exact
    # bytes() of the parts (what travels between processes) merge alike, in any shard order
    reports, _ = lib_merge([bytes(a) for a in reversed(arrs)])
    assert reports[0]["frag_bins"][0] == exact


def test_library_argument_errors():
    L = ksim.lib()
    one = (ksim.ReportPart * 1)()
    ptrs = (C.POINTER(ksim.ReportPart) * 17)(*[C.cast(one, C.POINTER(ksim.ReportPart))] * 17)
    out, pw = (ksim.Report * 1)(), (ksim.PowerReport * 1)()
    assert L.ksim_report_merge(None, 1, 1, out, pw) == ksim.KSIM_EINVAL
    assert L.ksim_report_merge(ptrs, 1, 1, None, pw) == ksim.KSIM_EINVAL
    assert L.ksim_report_merge(ptrs, 0, 1, out, pw) == ksim.KSIM_EINVAL
    assert L.ksim_report_merge(ptrs, 17, 1, out, pw) == ksim.KSIM_EINVAL
    assert L.ksim_report_merge(ptrs, 1, -1, out, pw) == ksim.KSIM_EINVAL
    assert L.ksim_report_merge(ptrs, 16, 1, out, None) == ksim.KSIM_OK
    with pytest.raises(ValueError):
        ksim.report_merge([])
    with pytest.raises(ValueError):
        ksim.report_merge([one, (ksim.ReportPart * 2)()])
    with pytest.raises(ValueError):
        ksim.report_merge([b"\0" * 207])
    # the null engine / null output checks of the device-side entry points come before any device work
    assert L.ksim_engine_get_report_parts(None, 0, one, 1) == ksim.KSIM_EINVAL
    assert L.ksim_shard_group_get_reports(None, 1, out, None, 1) == ksim.KSIM_EINVAL


def test_native_program_under_sanitizers(cases, tmp_path):
    # the same header in a stand-alone program built with -fsanitize=address,undefined: the 2000 records and the
    # exactness case, its own argument-error and size checks
    subprocess.run(["make", "-s", "-C", HERE], check=True)
    arrs_x, exact = exactness_case()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for world, arrs, _ in cases + [(3, arrs_x, None)]:
            f.write(struct.pack("<ii", world, len(arrs[0])))
            for a in arrs:
                f.write(bytes(a))
    p = subprocess.run([os.path.join(HERE, "report_merge_check"), src, dst], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines() == ["cases=17 records=2001", "ok"]
    raw = open(dst, "rb").read()
    rec = C.sizeof(ksim.Report) + C.sizeof(ksim.PowerReport)
    assert len(raw) == 2001 * rec
    off = 0
    for world, _, want in cases:
        for i, (wr, wp) in enumerate(want):
            r = ksim.Report.from_buffer_copy(raw, off)
            q = ksim.PowerReport.from_buffer_copy(raw, off + C.sizeof(ksim.Report))
            off += rec
            assert ksim.Engine._report_dicts([r], 1)[0] == wr, (world, i)
            assert ksim.Engine._power_dicts([q], 1)[0] == wp, (world, i)
    assert ksim.Report.from_buffer_copy(raw, off).frag_bins[0] == exact
