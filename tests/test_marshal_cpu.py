"""The Python marshaller of the report modules (sweepga_amd/_marshal.py) without a GPU and without a library call: host columns,
SwgRecords from numpy columns and from device tensors.  The tensors are stand-ins with the four methods the marshaller asks for."""
import numpy as np
import pytest

from sweepga_amd._lib import SwgRecords
from sweepga_amd._marshal import host_column, records_from_numpy, records_from_tensors

COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")


class FakeTensor:
    def __init__(self, ptr, numel, size=4, contiguous=True):
        self.ptr, self.n, self.size, self.contiguous = ptr, numel, size, contiguous

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n

    def element_size(self):
        return self.size

    def is_contiguous(self):
        return self.contiguous


def test_host_column_short_array_names_the_column():
    with pytest.raises(ValueError, match="^chain has fewer entries than records$"):
        host_column(np.zeros(2, dtype=np.uint32), np.uint32, 3, "chain")
    with pytest.raises(ValueError, match="^status has fewer entries than records$"):
        host_column([], np.uint8, 1, "status", optional=True)


def test_host_column_empty_gives_a_placeholder():
    a = host_column(np.zeros(0, dtype=np.uint8), np.uint8, 0, "status")
    assert a.dtype == np.uint8 and a.size == 1 and a[0] == 0 and a.ctypes.data != 0


def test_host_column_none():
    assert host_column(None, np.uint8, 5, "status", optional=True) is None
    with pytest.raises((TypeError, ValueError)):   # not optional: None is no column
        host_column(None, np.uint8, 5, "status")


def test_host_column_copies_what_is_not_contiguous_or_of_another_type():
    base = np.arange(10, dtype=np.uint32)
    a = host_column(base[::2], np.uint32, 5, "chain")
    assert a.flags["C_CONTIGUOUS"] and a.tolist() == [0, 2, 4, 6, 8] and not np.shares_memory(a, base)
    b = host_column(base, np.uint32, 10, "chain")
    assert b is base   # (nothing to convert: the caller's array itself)
    c = host_column([1, 0, 1], np.uint8, 3, "status")
    assert c.dtype == np.uint8 and c.tolist() == [1, 0, 1]


def test_records_from_numpy_dict():
    cols = {k: np.arange(3, dtype=np.int64) + 10 * j for j, k in enumerate(COLUMNS + ("matches", "block_len"))}
    cols["strand"] = np.array([0, 1, 0])
    rec, keep = records_from_numpy(cols, COLUMNS + ("strand",), 7, optional=("matches", "identity"))
    assert int(rec.n) == 3 and int(rec.n_seq) == 7
    names = COLUMNS + ("strand", "matches")
    assert len(keep) == len(names)
    for k, a in zip(names, keep):
        assert a.dtype == (np.uint8 if k == "strand" else np.uint32) and a.flags["C_CONTIGUOUS"]
        assert a.tolist() == np.asarray(cols[k]).tolist()
        assert getattr(rec, k) == a.ctypes.data, k
    assert not rec.block_len and not rec.identity   # (neither named nor, for identity, there)


def test_records_from_numpy_strand_apart_and_n_seq_from_the_ids():
    cols = {k: np.array([4, 9], dtype=np.uint32) for k in COLUMNS}
    rec, keep = records_from_numpy(cols, COLUMNS, None, strand=np.array([1, 0], dtype=np.uint8))
    assert int(rec.n) == 2 and int(rec.n_seq) == 10 and rec.strand == keep[-1].ctypes.data and keep[-1].dtype == np.uint8
    empty = {k: np.zeros(0, dtype=np.uint32) for k in COLUMNS}
    rec, keep = records_from_numpy(empty, COLUMNS, None, strand=np.zeros(0, dtype=np.uint8))
    assert int(rec.n) == 0 and int(rec.n_seq) == 1 and not rec.q_id and not rec.strand


def test_records_from_numpy_passes_a_struct_through():
    r = SwgRecords()
    r.n, r.n_seq = 5, 2
    rec, keep = records_from_numpy(r, COLUMNS, 99)
    assert rec is r and keep == [] and int(r.n_seq) == 2


def test_records_from_tensors():
    sizes = {**{k: 4 for k in COLUMNS}, "strand": 1}
    cols = {k: FakeTensor(0x1000 * (j + 1), 6) for j, k in enumerate(COLUMNS)}
    cols["strand"] = FakeTensor(0x9000, 6, size=1)
    rec = records_from_tensors(cols, sizes, 4)
    assert int(rec.n) == 6 and int(rec.n_seq) == 4 and rec.strand == 0x9000
    assert [getattr(rec, k) for k in COLUMNS] == [0x1000 * (j + 1) for j in range(6)]
    for bad, size in ((FakeTensor(0x2000, 5), 4), (FakeTensor(0x2000, 6, size=8), 4), (FakeTensor(0x2000, 6, contiguous=False), 4)):
        with pytest.raises(ValueError, match=f"^column t_id: a contiguous {size}-byte tensor of 6 entries is needed$"):
            records_from_tensors({**cols, "t_id": bad}, sizes, 4)
    with pytest.raises(ValueError, match="^column strand: a contiguous 1-byte tensor of 6 entries is needed$"):
        records_from_tensors({**cols, "strand": FakeTensor(0x9000, 6, size=4)}, sizes, 4)


def test_records_from_tensors_without_records():
    cols = {k: FakeTensor(0, 0) for k in COLUMNS}
    rec = records_from_tensors(cols, {k: 4 for k in COLUMNS}, 3)
    assert int(rec.n) == 0 and int(rec.n_seq) == 3 and not rec.q_id
