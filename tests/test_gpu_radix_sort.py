"""The library's own radix sort (csrc/radix_sort.hip: the sort behind voxel keys, the grid build's cell ids) against
torch.sort(stable=True): keys AND the order of equal keys' values, ragged sizes, every pass count, heavy duplicates."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


def run_sort(L, sp, keys, vals, bits):
    n = keys.numel()
    ka, va = keys.clone(), vals.clone()
    kb, vb = torch.empty_like(ka), torch.empty_like(va)
    ws = torch.empty(max(int(L.sp_internal_radix_sort_workspace_bytes(n)), 16), dtype=torch.uint8, device="cuda")
    in_b = C.c_int(-1)
    sp.check(L.sp_internal_radix_sort_u32(sp._ptr(ka), sp._ptr(kb), sp._ptr(va), sp._ptr(vb), n, bits, sp._ptr(ws), ws.numel(),
                                          C.byref(in_b), sp._stream()))
    torch.cuda.synchronize()
    return (kb, vb) if in_b.value == 1 else (ka, va)


@pytest.mark.parametrize("n,bits", [(1, 8), (63, 5), (4096, 8), (4097, 9), (100_003, 17), (1_000_000, 23), (1_000_000, 24),
                                    (262_144, 32), (3_000_001, 22)])
def test_radix_sort_matches_stable_torch_sort(sp, n, bits):
    L = sp._lib.lib()
    g = torch.Generator(device="cuda").manual_seed(n + bits)
    hi = (1 << bits) - 1
    keys = torch.randint(0, min(hi, 2**31 - 1) + 1, (n,), generator=g, device="cuda", dtype=torch.int64)
    if bits == 32:
        keys = keys * 2 + torch.randint(0, 2, (n,), generator=g, device="cuda", dtype=torch.int64)
    vals = torch.arange(n, device="cuda", dtype=torch.int32)
    ku = (keys & 0xFFFFFFFF).to(torch.int64)
    k_i32 = torch.where(ku >= 2**31, ku - 2**32, ku).to(torch.int32)  # same bits as the unsigned key
    sk, sv = run_sort(L, sp, k_i32, vals, bits)
    ref_k, ref_order = torch.sort(ku, stable=True)
    got_k = sk.to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got_k, ref_k)
    assert torch.equal(sv.to(torch.int64), ref_order)  # stability: equal keys keep their input order


def test_radix_sort_heavy_duplicates_and_presorted(sp):
    L = sp._lib.lib()
    n = 500_000
    keys = (torch.arange(n, device="cuda") % 7).to(torch.int32)  # seven distinct keys: whole tiles of one digit
    vals = torch.arange(n, device="cuda", dtype=torch.int32)
    sk, sv = run_sort(L, sp, keys, vals, 3)
    ref_k, ref_order = torch.sort(keys.to(torch.int64), stable=True)
    assert torch.equal(sk.to(torch.int64), ref_k) and torch.equal(sv.to(torch.int64), ref_order)
    keys = torch.arange(n, device="cuda", dtype=torch.int32)  # already sorted, 19 bits
    sk, sv = run_sort(L, sp, keys, vals, 19)
    assert torch.equal(sk, keys) and torch.equal(sv, vals)


# ------------------------------------------------------------------ every branch, directly
# radix_sort_pairs has four dispatch branches — 8- or 9-bit digits (9 where that saves a pass), with the scan launch or, up to
# 64 tiles of 2048 keys, without it (FOLD) — for two key types, a partial sort (first_bit > 0) and a first pass whose tile
# histograms the caller supplies. Every case below is compared with numpy's stable argsort of the sorted bit field: the keys
# come back with ALL their bits, the values are the stable order itself. Each call runs twice (identical bytes) on a workspace
# filled with 0xAB (nothing may depend on what it held).
SIZES = [2047, 2048, 2049, 131_072, 131_073, 526_337]  # one tile | a full tile | 2 tiles, the last of one key | 64 tiles, the last
# fold | 65 tiles, the first scan launch | 258 tiles: rs_scan_kernel's carry loop runs a third chunk, of two tiles


def digit_bits(span):
    return 9 if -(-span // 9) < -(-span // 8) else 8


@functools.lru_cache(maxsize=None)
def random_keys(n, width):
    rng = np.random.default_rng(1000 * width + n % 997)
    k = rng.integers(0, 2**64, n, dtype=np.uint64, endpoint=False)
    return k if width == 64 else (k >> np.uint64(32)).astype(np.uint32)


def field_of(keys, bits, first_bit):
    return (keys.astype(np.uint64) >> np.uint64(first_bit)) & np.uint64(2 ** (bits - first_bit) - 1)


def reference(keys, bits, first_bit=0):
    order = np.argsort(field_of(keys, bits, first_bit), kind="stable")
    return keys[order], order.astype(np.uint32)


def device_sort(L, sp, keys, bits, first_bit=0, hist=None):
    """One call of the u32 (_ex) or u64 entry on fresh copies: (rc, result_in_b, [keys_a, vals_a, keys_b, vals_b] on the host)."""
    n, wide = len(keys), keys.dtype == np.uint64
    ka = torch.from_numpy(keys.view(np.int64 if wide else np.int32).copy()).cuda()
    va = torch.arange(n, device="cuda", dtype=torch.int32)
    kb, vb = torch.full_like(ka, -1), torch.full_like(va, -1)
    nbytes = int(L.sp_internal_radix_sort_workspace_bytes(n))
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    if hist is not None:
        ws[:hist.nbytes] = torch.from_numpy(hist.view(np.uint8)).cuda()
    in_b = C.c_int(-1)
    if wide:
        assert first_bit == 0 and hist is None
        rc = L.sp_internal_radix_sort_u64(sp._ptr(ka), sp._ptr(kb), sp._ptr(va), sp._ptr(vb), n, bits, sp._ptr(ws), nbytes,
                                          C.byref(in_b), sp._stream())
    else:
        rc = L.sp_internal_radix_sort_u32_ex(sp._ptr(ka), sp._ptr(kb), sp._ptr(va), sp._ptr(vb), n, bits, first_bit,
                                             int(hist is not None), sp._ptr(ws), nbytes, C.byref(in_b), sp._stream())
    torch.cuda.synchronize()
    host = [t.cpu().numpy().view(keys.dtype if i % 2 == 0 else np.uint32) for i, t in enumerate((ka, va, kb, vb))]
    return rc, in_b.value, host


def sorted_pair(L, sp, keys, bits, first_bit=0, hist=None):
    """The sorted (keys, values) of two identical calls, which must agree byte for byte."""
    out = []
    for _ in range(2):
        rc, in_b, host = device_sort(L, sp, keys, bits, first_bit, hist)
        sp.check(rc)
        assert in_b in (0, 1)
        out.append((host[2], host[3]) if in_b else (host[0], host[1]))
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    return out[0]


def check_sort(L, sp, keys, bits, first_bit=0):
    got_k, got_v = sorted_pair(L, sp, keys, bits, first_bit)
    ref_k, ref_v = reference(keys, bits, first_bit)
    assert np.array_equal(got_k, ref_k)  # every bit of the key, the ignored ones included
    assert np.array_equal(got_v, ref_v)  # stability: equal fields keep their input order


@pytest.mark.parametrize("bits", [1, 8, 9, 16, 17, 18, 25, 27, 32])
@pytest.mark.parametrize("n", SIZES)
def test_radix_sort_u32_every_branch(sp, n, bits):
    # fold/8: bits 8, 16, 32 up to 131 072 | fold/9: 9, 17, 18, 25, 27 up to 131 072 | scan/8 and scan/9: the same above it;
    # one to four passes, a narrower last digit (1, 17, 25 bits)
    check_sort(sp._lib.lib(), sp, random_keys(n, 32), bits)


@pytest.mark.parametrize("bits,first_bit", [(20, 4), (24, 8), (17, 1), (32, 16), (27, 2), (18, 9)])
@pytest.mark.parametrize("n", [2049, 131_073, 526_337])
def test_radix_sort_u32_partial_sort_by_a_bit_field(sp, n, bits, first_bit):
    check_sort(sp._lib.lib(), sp, random_keys(n, 32), bits, first_bit)


def test_radix_sort_u32_empty_bit_field_touches_nothing(sp):
    keys = random_keys(2049, 32)
    rc, in_b, (ka, va, kb, vb) = device_sort(sp._lib.lib(), sp, keys, 12, 12)
    assert rc == 0 and in_b == 0
    assert np.array_equal(ka, keys) and np.array_equal(va, np.arange(2049, dtype=np.uint32))
    assert np.all(kb == 0xFFFFFFFF) and np.all(vb == 0xFFFFFFFF)


def five_high_words(n):
    k = random_keys(n, 64)
    high = np.random.default_rng(5).integers(0, 2**32, 5, dtype=np.uint64)
    return (high[k % np.uint64(5)] << np.uint64(32)) | (k >> np.uint64(32))


@pytest.mark.parametrize("keyset", ["random", "five_high_words"])
@pytest.mark.parametrize("bits", [1, 9, 33, 48, 63, 64])
@pytest.mark.parametrize("n", [2049, 131_072, 131_073])
def test_radix_sort_u64_every_branch(sp, n, bits, keyset):
    # fold/8: bits 1, 48, 64 up to 131 072 | fold/9: 9, 33, 63 | scan/8 and scan/9: the same at 131 073
    keys = random_keys(n, 64) if keyset == "random" else five_high_words(n)
    check_sort(sp._lib.lib(), sp, keys, bits)


def duplicate_keys(kind, width, n, bits, first_bit):
    rng = np.random.default_rng(len(kind) + bits)
    rand = random_keys(n, width).astype(np.uint64)
    span = bits - first_bit
    fmask = np.uint64((2**span - 1) << first_bit)
    outside = rand & ~fmask
    if kind == "all_equal":
        k = np.full(n, rand[0])
    elif kind == "equal_in_field":  # the sort may not move anything; the bits outside the field tell the rows apart
        k = outside | (rand[0] & fmask)
    elif kind == "three_digits":  # three distinct digits in every pass (two where the last digit is one bit wide)
        digit, field = digit_bits(span), np.zeros(n, np.uint64)
        for shift in range(0, span, digit):
            width_p = min(digit, span - shift)
            choice = rng.choice(1 << width_p, size=min(3, 1 << width_p), replace=False).astype(np.uint64)
            field |= choice[rng.integers(0, len(choice), n)] << np.uint64(shift)
        k = outside | (field << np.uint64(first_bit))
    else:
        k = rand[np.argsort(field_of(rand, bits, first_bit), kind="stable")]
        if kind == "reversed":
            k = k[::-1].copy()
        else:
            assert kind == "presorted"
    return k.astype(np.uint64 if width == 64 else np.uint32)


@pytest.mark.parametrize("kind", ["all_equal", "equal_in_field", "three_digits", "presorted", "reversed"])
@pytest.mark.parametrize("width,bits,first_bit", [(32, 32, 0), (32, 24, 8), (32, 18, 0), (64, 48, 0), (64, 63, 0)])
def test_radix_sort_duplicates_and_whole_wave_digits(sp, width, bits, first_bit, kind):
    # rs_count_kernel adds a whole wave to one counter when its 64 keys share the digit: equal keys, the high digits of a sorted run
    check_sort(sp._lib.lib(), sp, duplicate_keys(kind, width, 131_073, bits, first_bit), bits, first_bit)


@pytest.mark.parametrize("bits", [8, 9, 18, 24])
@pytest.mark.parametrize("n", [2049, 131_072, 131_073])
def test_radix_sort_first_pass_histograms_from_the_caller(sp, n, bits):
    # the radix_first_pass() contract (radix_sort.h): hist[digit * tiles + tile] at the start of the workspace
    L = sp._lib.lib()
    keys = random_keys(n, 32)
    out4 = (C.c_uint * 4)()
    L.sp_internal_radix_first_pass(n, bits, out4)
    tiles, tile_keys, digit, mask = (int(v) for v in out4)
    d = (keys & np.uint32(mask)).astype(np.int64)
    hist = np.bincount(d * tiles + np.arange(n) // tile_keys, minlength=(1 << digit) * tiles).astype(np.uint32)
    assert hist.sum() == n and len(hist) == (1 << digit) * tiles
    plain_k, plain_v = sorted_pair(L, sp, keys, bits)
    ready_k, ready_v = sorted_pair(L, sp, keys, bits, hist=hist)
    assert ready_k.tobytes() == plain_k.tobytes() and ready_v.tobytes() == plain_v.tobytes()
    ref_k, ref_v = reference(keys, bits)
    assert np.array_equal(ready_k, ref_k) and np.array_equal(ready_v, ref_v)


def test_radix_sort_left_no_device_error(sp):
    # (the file's last call) a look-back guard that tripped in an earlier kernel comes back from the NEXT library call
    check_sort(sp._lib.lib(), sp, random_keys(2049, 32), 8)
