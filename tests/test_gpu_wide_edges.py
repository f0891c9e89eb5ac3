"""The u64 -> u32 rebasing rule at its edges on both entry points that take u64 columns: swg_filter64 (host columns, rebased by
host threads: csrc/host/rebase.h) and swg_filter_device64 (device columns, rebased by seq_lo / rebase / axis_lo / axis_rebase of
csrc/swg_filter.hip).  The named cases of tests/wide_cases.py, each against tests/wide_model.py: the return code; for a refusal
the error text of both paths, which must be the same and name the model's record and field; for an accepted case status and
chain numbers of both paths against each other and against the oracle on the unrebased u64 records, under two flag sets."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import orc
from tests import wide_cases as wc
from tests import wide_model as wm
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu

SWG_ERR_INVALID, SWG_ERR_RANGE = -1, -5   # include/sweepga_gpu.h
FLAG_SETS = [dict(),
             dict(mapping_filter_mode="OneToOne", scaffold_filter_mode="OneToOne", scaffold_gap=5_000, min_scaffold_length=1_000,
                  scaffold_max_deviation=30_000)]


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def _configs(sw):
    out = []
    for kw in FLAG_SETS:
        cfg = sw.FilterConfig(**{k: (getattr(sw.FilterMode, v) if isinstance(v, str) else v) for k, v in kw.items()})
        ocfg = orc.Config(**{k: (int(getattr(sw.FilterMode, v)) if isinstance(v, str) else v) for k, v in kw.items()})
        out.append((cfg.to_c(False, False), ocfg))
    return out


def _columns(c):
    """The case as the arrays of swg_records64.  The genome table gets one entry more than n_seq, a zero: an id out of range in
    these cases is n_seq itself, so even code that followed it would stay inside the table."""
    n = c.n
    a = {"q_id": np.array(c.q_id, dtype=np.uint32), "t_id": np.array(c.t_id, dtype=np.uint32)}
    for f, k in enumerate(("q_start", "q_end", "t_start", "t_end", "matches", "block_len")):
        a[k] = np.array(c.cols[f], dtype=np.uint64)
    a["identity"] = np.array([min(c.cols[4][i] / max(c.cols[5][i], 1), 1.0) for i in range(n)], dtype=np.float64)
    a["strand"] = np.zeros(n, dtype=np.uint8)
    a["genome"] = np.array(list(c.genome) + [0], dtype=np.uint32)
    assert len(a["genome"]) == c.n_seq + 1 and max(c.q_id + c.t_id + [0]) <= c.n_seq
    return {k: np.ascontiguousarray(v) for k, v in a.items()}


def _records(c, a, ptr):
    from sweepga_amd._lib import SwgRecords
    r = SwgRecords()
    r.n = c.n
    for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "identity", "matches", "block_len", "strand"):
        setattr(r, k, ptr(a[k]))
    r.n_seq = c.n_seq
    r.seq_genome_last = r.seq_genome_two = ptr(a["genome"])
    r.n_genome_last = r.n_genome_two = c.n_genome
    return r


def _oracle_records(c, a):
    u = lambda f: np.array(c.cols[f], dtype=np.uint64)   # noqa: E731
    names = c.names
    return orc.Records([names[i] for i in c.q_id], [names[i] for i in c.t_id], u(0), u(1), u(2), u(3), u(5), a["identity"], u(4),
                       np.full(c.n, ord("+"), dtype=np.uint8), np.arange(c.n, dtype=np.uint64))


def _run_case(sw, c, configs):
    from sweepga_amd._lib import SwgStats
    ctx = sw.default_context()
    lib = ctx.lib
    want = c.result
    want_rc = {"ok": 0, "invalid": SWG_ERR_INVALID, "range": SWG_ERR_RANGE}[want[0]]
    a = _columns(c)
    n = c.n
    hip = Hip()
    try:
        host_rec = _records(c, a, lambda v: v.ctypes.data)
        dev_rec = _records(c, a, hip.up)
        d_status, d_chain = hip.alloc(n), hip.alloc(4 * n)
        orec = _oracle_records(c, a) if (want[0] == "ok" and c.modelled and n) else None
        for cc, ocfg in configs:
            status, chain, stats = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32), SwgStats()
            rc_h = lib.swg_filter64(ctx.handle, C.byref(host_rec), C.byref(cc), C.c_void_p(status.ctypes.data),
                                    C.c_void_p(chain.ctypes.data), C.byref(stats))
            err_h = lib.swg_last_error(ctx.handle).decode() if rc_h else ""
            assert rc_h == want_rc, (c.name, "host columns", rc_h, err_h, want[:3])
            rc_d = lib.swg_filter_device64(ctx.handle, C.byref(dev_rec), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain),
                                           C.byref(stats))
            err_d = lib.swg_last_error(ctx.handle).decode() if rc_d else ""
            assert rc_d == want_rc, (c.name, "device columns", rc_d, err_d, want[:3])
            if want[0] != "ok":
                assert err_h == err_d, (c.name, err_h, err_d)
                assert err_h.startswith(f"record {want[1]}: "), (c.name, err_h, want)
                if want[0] == "range":
                    assert wm.FIELDS[want[2]] in err_h and not any(x in err_h for x in wm.FIELDS if x != wm.FIELDS[want[2]]), (c.name, err_h)
                continue
            ctx.synchronize()
            d_st, d_ch = hip.down(d_status, np.uint8, n), hip.down(d_chain, np.uint32, n)
            assert np.array_equal(status[:n], d_st) and np.array_equal(chain[:n], d_ch), (c.name, "host columns != device columns")
            if orec is not None:
                ost, och = orc.apply_filters(ocfg, orec)
                assert np.array_equal(d_st, ost), (c.name, int((d_st != ost).sum()))
                assert np.array_equal(d_ch, och), (c.name, int((d_ch != och).sum()))
    finally:
        hip.free()


def _run_group(sw, name):
    t0 = time.perf_counter()
    cases = wc.group(name)
    configs = _configs(sw)
    for c in cases:
        _run_case(sw, c, configs)
    print(f"{name}: {len(cases)} cases in {time.perf_counter() - t0:.2f} s")


def test_boundary(sw):
    """2^32 - 1 above a sequence's smallest coordinate is accepted (0xFFFFFFFF), 2^32 is refused with that record and field: each
    coordinate field, the record at index 0, 63, 64 and n - 1 of n = 1 .. 3 * EW + 7 records; reversed intervals; matches and block
    length; coordinates at the top of u64; no records at all."""
    _run_group(sw, "boundary")


def test_wavefronts(sw):
    """seq_min_atomic's one-atomic-per-wavefront path: 64 records of one (query, target) with the minimum in lane 0, 31 and 63; one
    axis uniform and the other mixed; a last wavefront with one live lane; a sequence named only as a target; unnamed sequences.
    Every stretch is exactly 2^32 - 1 wide, so a constant off in either direction is a refusal."""
    _run_group(sw, "wavefronts")


def test_two_axes(sw):
    """The constants per (sequence, genome of the other side): a self mapping with its two stretches 2^33 apart, a sequence against
    two genomes 2^33 apart, the same with one segment too wide (the axis attempt's record, not the first attempt's), the tables'
    limit of 2^24 cells from both sides, a genome table entry out of range."""
    _run_group(sw, "two_axes")


def test_precedence(sw):
    """An id out of range wins wherever it sits -- also behind a record whose span is too wide, where one shared error word used to
    hide it and the axis kernels followed the id.  The case whose wide segment cannot be fixed runs first: before the fix it came
    back as SWG_ERR_RANGE, which fails here without any kernel having followed a bad id."""
    _run_group(sw, "precedence")
