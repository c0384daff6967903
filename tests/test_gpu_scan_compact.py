"""The one-launch exclusive scan and the fused compaction by flags (csrc/radix_sort.hip, the decoupled look-back of
csrc/sp_lookback.h) on their own, against numpy: np.cumsum in uint64 and boolean indexing, compared exactly. Sizes either side
of a tile of 2048, more than the 64 tiles one look-back step covers, in place, with and without the optional outputs, rows that
take the word-by-word move, and a workspace filled with 0xAB (nothing may depend on what it held)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0xCD


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ exclusive_scan_u32
def device_scan(L, sp, values, in_place, with_total):
    n = len(values)
    d_in = dev(values.view(np.int32))
    d_out = d_in if in_place else torch.full_like(d_in, -1)
    total = torch.full((1,), -1, dtype=torch.int32, device="cuda") if with_total else None
    nbytes = int(L.sp_internal_exclusive_scan_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    sp.check(L.sp_internal_exclusive_scan_u32(sp._ptr(d_in) if n else None, sp._ptr(d_out) if n else None, n, sp._ptr(total),
                                              sp._ptr(ws), nbytes, sp._stream()))
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), values)  # the input is read only
    return d_out.cpu().numpy().view(np.uint32), (int(total.cpu().numpy().view(np.uint32)[0]) if with_total else None)


def check_scan(L, sp, values):
    inclusive = np.cumsum(values, dtype=np.uint64)
    ref = np.concatenate((np.zeros(1, np.uint64), inclusive[:-1])) if len(values) else inclusive  # shifted by one place
    ref_total = int(inclusive[-1]) if len(values) else 0
    assert ref_total < 2**30
    for in_place in (False, True):
        for with_total in (True, False):
            got, total = device_scan(L, sp, values, in_place, with_total)
            assert np.array_equal(got.astype(np.uint64), ref), (in_place, with_total)
            if with_total:
                assert total == ref_total, (in_place, with_total)


def scan_input(kind, n):
    if kind == "ones":
        return np.ones(n, np.uint32)
    if kind == "zeros":
        return np.zeros(n, np.uint32)
    return np.random.default_rng(n).integers(0, 8, n, dtype=np.uint32)


# 0: total_out becomes 0 | 1 | either side of a tile | 64 tiles: one look-back step reaches tile 0 | 65 and 489 tiles: more steps
@pytest.mark.parametrize("kind", ["ones", "zeros", "random_0_7"])
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 131_072, 131_073, 1_000_003])
def test_exclusive_scan_matches_cumsum(sp, n, kind):
    check_scan(sp._lib.lib(), sp, scan_input(kind, n))


def test_exclusive_scan_largest_legal_total(sp):
    # the state word of a tile packs a 2-bit flag with a 30-bit sum: 2^30 - 1 is the largest total it holds. Non-zero values in
    # the first, a middle and the last tile (of one value) only: tile 64's look-back crosses 31 tiles of zeros
    n = 131_073
    v = np.zeros(n, np.uint32)
    v[5], v[2047], v[32 * 2048 + 77], v[n - 1] = 2**29, 2**28 - 1, 2**27, 2**27
    assert int(v.sum(dtype=np.uint64)) == 2**30 - 1
    check_scan(sp._lib.lib(), sp, v)


# ------------------------------------------------------------------ compaction by flags
ROW_BYTES = [4, 8, 12, 16, 20, 32, 48, 64]
COMPACT_SIZES = [1, 2047, 2048, 2049, 131_073]
PATTERNS = ["all", "none", "first", "last", "half", "values_0_1_2_255"]


def make_flags(pattern, n):
    f = np.zeros(n, np.uint8)
    if pattern == "all":
        f[:] = 1
    elif pattern == "first":
        f[0] = 1
    elif pattern == "last":
        f[-1] = 1
    elif pattern == "half":
        f = np.random.default_rng(n).integers(0, 2, n, dtype=np.uint8)
    elif pattern == "values_0_1_2_255":  # only INCLUDE_FLAG == 1 keeps a row
        f = np.array([0, 1, 2, 255], np.uint8)[np.random.default_rng(n + 1).integers(0, 4, n)]
    else:
        assert pattern == "none"
    return f


@functools.lru_cache(maxsize=None)
def source_rows(n, row_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, row_bytes), dtype=np.uint8)


class Slot:
    """One attribute array of a compaction call: `rows` (n, row_bytes) on the host, uploaded `src_shift` bytes past a 256-byte
    boundary, an output buffer pre-filled with SENTINEL that starts `dst_shift` bytes past one (None: a null rows_out slot)."""

    def __init__(self, rows, src_shift=0, dst_shift=0):
        self.rows, self.nbytes, self.dst_shift = rows, rows.size, dst_shift
        self.src_buf = torch.full((self.nbytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.src = self.src_buf[src_shift:src_shift + self.nbytes]
        self.src.copy_(dev(rows.reshape(-1)))
        self.dst_buf = self.dst = None
        if dst_shift is not None:
            self.dst_buf = torch.full((self.nbytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            self.dst = self.dst_buf[dst_shift:dst_shift + self.nbytes]
        assert self.src_buf.data_ptr() % 256 == 0 and (self.dst_buf is None or self.dst_buf.data_ptr() % 256 == 0)

    def check(self, keep):
        if self.dst_buf is None:
            return
        got = self.dst_buf.cpu().numpy()
        kept = self.rows[keep].reshape(-1)  # the reference: numpy boolean indexing
        lo = self.dst_shift
        assert got[lo:lo + kept.size].tobytes() == kept.tobytes()
        assert np.all(got[:lo] == SENTINEL) and np.all(got[lo + kept.size:] == SENTINEL)  # rows at and past the count: untouched
        assert np.array_equal(self.src.cpu().numpy(), self.rows.reshape(-1))


def run_compact(L, sp, slots, flags, want_idx, single=False):
    n, na = len(flags), len(slots)
    d_flags = dev(flags)
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda") if want_idx else None
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nbytes = int(L.sp_compact_workspace_bytes(n))
    ws = torch.full((max(nbytes, 16),), 0xAB, dtype=torch.uint8, device="cuda")
    if single:
        (s,) = slots
        rc = L.sp_compact_by_flags(sp._ptr(s.src), n, s.rows.shape[1], sp._ptr(d_flags), sp._ptr(s.dst), sp._ptr(idx), sp._ptr(count),
                                   sp._ptr(ws), nbytes, sp._stream())
    else:
        rows = (C.c_void_p * na)(*[s.src.data_ptr() for s in slots])
        outs = (C.c_void_p * na)(*[None if s.dst is None else s.dst.data_ptr() for s in slots])
        sizes = (C.c_size_t * na)(*[s.rows.shape[1] for s in slots])
        rc = L.sp_compact_by_flags_multi(rows, sizes, outs, na, n, sp._ptr(d_flags), sp._ptr(idx), sp._ptr(count), sp._ptr(ws), nbytes,
                                         sp._stream())
    sp.check(rc)
    torch.cuda.synchronize()
    keep = flags == 1
    assert int(count.cpu()[0]) == int(keep.sum())
    for s in slots:
        s.check(keep)
    if want_idx:
        assert np.array_equal(idx.cpu().numpy(), np.where(keep, np.cumsum(keep, dtype=np.int64) - 1, -1))
    assert np.array_equal(d_flags.cpu().numpy(), flags)


@pytest.mark.parametrize("want_idx", [True, False])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compact_sixteen_arrays_in_one_call(sp, n, pattern, want_idx):
    # rows of whole 16-byte quads (16, 32, 48, 64 bytes) move as quads, the others (4, 8, 12, 20) word by word
    slots = [Slot(source_rows(n, ROW_BYTES[a % 8], a)) for a in range(16)]
    run_compact(sp._lib.lib(), sp, slots, make_flags(pattern, n), want_idx)


@pytest.mark.parametrize("want_idx", [True, False])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compact_rows_off_a_16_byte_boundary(sp, n, pattern, want_idx):
    # 16-byte rows whose source, or whose destination, starts 4 bytes past a 16-byte boundary: the quad move would fault or
    # tear; both in one sp_compact_by_flags_multi call beside an aligned array, then each alone through sp_compact_by_flags
    L, flags = sp._lib.lib(), make_flags(pattern, n)
    make = lambda: [Slot(source_rows(n, 16, 100), src_shift=4), Slot(source_rows(n, 16, 101), dst_shift=4),  # noqa: E731
                    Slot(source_rows(n, 16, 102))]
    run_compact(L, sp, make(), flags, want_idx)
    for s in make():
        run_compact(L, sp, [s], flags, want_idx, single=True)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", COMPACT_SIZES)
def test_compact_skips_null_output_slots(sp, n, pattern):
    # an attribute whose rows_out slot is null is only counted: the arrays around it come out as if it were not there
    slots = [Slot(source_rows(n, 16, 0)), Slot(source_rows(n, 12, 1), dst_shift=None), Slot(source_rows(n, 20, 2)),
             Slot(source_rows(n, 64, 3), dst_shift=None), Slot(source_rows(n, 4, 4))]
    run_compact(sp._lib.lib(), sp, slots, make_flags(pattern, n), True)


def test_compact_argument_errors(sp):
    L = sp._lib.lib()
    n = 2049
    flags = dev(make_flags("half", n))
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = int(L.sp_compact_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    src = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    dst = torch.full_like(src, SENTINEL)

    def call(na, row_bytes, ws_bytes):
        rows, outs = (C.c_void_p * 17)(*[src.data_ptr()] * 17), (C.c_void_p * 17)(*[dst.data_ptr()] * 17)
        sizes = (C.c_size_t * 17)(*[row_bytes] * 17)
        return L.sp_compact_by_flags_multi(rows, sizes, outs, na, n, sp._ptr(flags), None, sp._ptr(count), sp._ptr(ws), ws_bytes,
                                           sp._stream())

    assert call(0, 16, nbytes) == 1 and call(17, 16, nbytes) == 1  # SP_ERR_INVALID_ARGUMENT
    assert call(1, 6, nbytes) == 1
    assert L.sp_last_error().decode() == "[FilterByFlags] row_bytes must be a positive multiple of 4 and n < 2^30"
    assert call(1, 16, nbytes - 1) == 1
    assert L.sp_last_error().decode() == "[FilterByFlags] workspace too small (sp_compact_workspace_bytes)"
    torch.cuda.synchronize()
    assert np.all(dst.cpu().numpy() == SENTINEL)  # a refused call launches nothing
    assert call(1, 16, nbytes) == 0


def test_scan_and_compaction_left_no_device_error(sp):
    # (the file's last call) a look-back guard that tripped in an earlier kernel comes back from the NEXT library call
    check_scan(sp._lib.lib(), sp, scan_input("ones", 2049))
