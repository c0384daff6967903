"""block_reduce_store (csrc/registration_device.h), the workgroup reduction that ends every launch of the registration kernels,
on its own through sp_internal_block_reduce: the partial row must be, BIT FOR BIT, what the DPP ladder gives that the reduction
was first written as, emulated here in NumPy float32 as written: an inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4,
8, lanes shifted in from outside the row read 0), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3, lane 63's
value per wave, then the waves in order added to 0. The expected row never comes from the function under test. So that the
comparison cannot pass vacuously, a left-to-right sum and a balanced tree with its levels reversed are computed on the same
inputs and must differ from the expected row for more than half of the random sums (on the CPU: about 77 % and 66 %)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WAVE, ROW_WORDS, DRAWS = 64, 32, 64
BLOCKS, NVS = (64, 256, 1024), (28, 1)
f32 = np.float32


@pytest.fixture(scope="module")
def sp():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (no CPU fallback exists)")
    import sycl_points_amd.api as api

    return api


# ----------------------------------------------------------------------------------------------- the ladder, as written

def row_shr_or_zero(v, n):
    """DPP row_shr:n with bound_ctrl: lane l of a row of 16 reads lane l - n of the same row, 0 from outside it. v: (..., 64)."""
    out = np.zeros_like(v)
    lane = np.arange(WAVE)
    ok = (lane % 16) >= n
    out[..., ok] = v[..., lane[ok] - n]
    return out


def row_bcast_or_zero(v, src_lane_of_row, rows):
    """DPP row_bcast with a row mask: the rows in `rows` read one lane (given per row), every other row gets the old value 0."""
    out = np.zeros_like(v)
    for r in rows:
        out[..., 16 * r:16 * r + 16] = v[..., src_lane_of_row[r]:src_lane_of_row[r] + 1]
    return out


def ladder_lane63(v):
    """wave_sum_to_lane63 on (..., 64) lanes, float32 or uint32: the value lane 63 ends with."""
    v = v.copy()
    for n in (1, 2, 4, 8):
        v = v + row_shr_or_zero(v, n)
    v = v + row_bcast_or_zero(v, {1: 15, 3: 47}, (1, 3))   # row_bcast:15, row_mask 0xa: lane 15 of the row before
    v = v + row_bcast_or_zero(v, {2: 31, 3: 31}, (2, 3))   # row_bcast:31, row_mask 0xc: lane 31
    return v[..., WAVE - 1]


def waves_in_order(per_wave):
    """The second stage: s = 0; s += wave 0; s += wave 1; ... per_wave: (..., waves)."""
    s = np.zeros(per_wave.shape[:-1], dtype=per_wave.dtype)
    for w in range(per_wave.shape[-1]):
        s = s + per_wave[..., w]
    return s


def expected_rows(vals, cnts):
    """vals: (draws, block, nv) float32, cnts: (draws, block, 2) uint32 -> (draws, 32) uint32 words of the partial row."""
    d, block, nv = vals.shape
    with np.errstate(all="ignore"):
        sums = waves_in_order(ladder_lane63(vals.reshape(d, block // WAVE, WAVE, nv).transpose(0, 3, 1, 2)))  # (d, nv)
        ints = waves_in_order(ladder_lane63(cnts.reshape(d, block // WAVE, WAVE, 2).transpose(0, 3, 1, 2)))   # (d, 2) uint32, wraps
    row = np.zeros((d, ROW_WORDS), dtype=np.uint32)
    row[:, :nv] = sums.astype(f32).view(np.uint32)
    row[:, nv] = ints[:, 0]                                  # the count: its bit pattern
    row[:, nv + 1] = ints[:, 1].astype(f32).view(np.uint32)  # the second integer: its value as a float
    return row


# ------------------------------------------------------------------------------- two other orders, for the vacuity guard

def left_to_right(vals):
    d, block, nv = vals.shape
    v = vals.reshape(d, block // WAVE, WAVE, nv)
    s = v[:, :, 0, :].copy()
    for l in range(1, WAVE):
        s = s + v[:, :, l, :]
    return waves_in_order(s.transpose(0, 2, 1))


def reversed_tree(vals):
    d, block, nv = vals.shape
    v = vals.reshape(d, block // WAVE, WAVE, nv).copy()
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o, :]
    return waves_in_order(v[:, :, 0, :].transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------ the probe

def run_probe(sp, vals, cnts):
    """One launch per draw; all draws are uploaded at once. -> (draws, 32) uint32."""
    d, block, nv = vals.shape
    dv, dc = torch.from_numpy(np.ascontiguousarray(vals)).cuda(), torch.from_numpy(cnts.view(np.int32).copy()).cuda()
    out = torch.full((d, ROW_WORDS), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    L = sp._lib.lib()
    for i in range(d):
        sp.check(L.sp_internal_block_reduce(sp._ptr(dv[i]), sp._ptr(dc[i]), block, nv, sp._ptr(out[i]), sp._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def random_inputs(block, nv, draws=DRAWS):
    """Every lane value is standard_normal x 10^k, k uniform in -6 .. 5: sums whose bits depend on the order of the additions."""
    rng = np.random.default_rng(20240 + 31 * block + nv)
    vals = (rng.standard_normal((draws, block, nv)) * 10.0 ** rng.integers(-6, 6, (draws, block, nv))).astype(f32)
    cnts = rng.integers(0, 1 << 12, (draws, block, 2), dtype=np.uint32)
    return vals, cnts


def assert_rows_equal(got, want, nv, nan_slots=()):
    for e in range(ROW_WORDS):
        if e in nan_slots:
            assert np.isnan(got[:, e].view(f32)).all() and np.isnan(want[:, e].view(f32)).all(), e
        else:
            bad = np.flatnonzero(got[:, e] != want[:, e])
            assert bad.size == 0, (f"word {e} of the row (nv {nv}): draw {bad[:4]}: got {got[bad[:4], e].view(f32)} "
                                   f"want {want[bad[:4], e].view(f32)}")


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("block", BLOCKS)
def test_random_rows_are_the_ladders_bits(sp, block, nv):
    vals, cnts = random_inputs(block, nv)
    want = expected_rows(vals, cnts)
    # the guard: on these inputs another order of the same additions gives other bits for most sums
    for name, other in (("left to right", left_to_right), ("levels reversed", reversed_tree)):
        differs = np.mean(other(vals).astype(f32).view(np.uint32) != want[:, :nv])
        print(f"block {block} nv {nv}: {name} differs from the ladder in {100 * differs:.0f} % of {DRAWS * nv} sums")
        assert differs > 0.5, (name, differs)
    assert_rows_equal(run_probe(sp, vals, cnts), want, nv)


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("block", BLOCKS)
def test_special_values(sp, block, nv):
    rng = np.random.default_rng(7 + block + nv)
    base, cnts = random_inputs(block, nv, draws=8)
    cases, nan_slots = [], []
    zero = np.zeros((block, nv), dtype=f32)
    cases.append(zero)                                                          # 0: every lane +0
    cases.append(-zero)                                                         # 1: every lane -0
    cases.append(np.where(rng.random((block, nv)) < 0.5, zero, -zero))          # 2: both zeros mixed
    one_neg = -zero                                                             # 3: -0 everywhere but one lane per value
    one_neg[rng.integers(0, block, nv), np.arange(nv)] = 0.0
    cases.append(one_neg)
    with_inf = base[4].copy()                                                   # 4: one lane inf (another value: -inf)
    with_inf[rng.integers(0, block), 0] = np.inf
    with_inf[rng.integers(0, block), nv - 1] = -np.inf if nv > 1 else np.inf
    cases.append(with_inf)
    with_nan = base[5].copy()                                                   # 5: one lane NaN, in value 0 only
    with_nan[rng.integers(0, block), 0] = np.nan
    cases.append(with_nan)
    with np.errstate(over="ignore"):
        cases.append(base[6] * f32(1e30))                                       # 6: sums that overflow to inf (or inf - inf)
    cases.append(base[7])                                                       # 7: plain, with the large counters below
    vals = np.stack(cases).astype(f32)
    # counters up to 2^24 per lane: 1024 lanes of them pass 2^32, and the sum must wrap as a uint32 does
    cnts[6:] = rng.integers((1 << 24) - 4096, (1 << 24) + 1, (2, block, 2), dtype=np.uint32)
    cnts[0] = 0
    want = expected_rows(vals, cnts)
    got = run_probe(sp, vals, cnts)
    # NaN: by NaN-ness only (the payload may depend on the order of the operands); case 6 may make NaN from inf - inf
    isn = np.isnan(want.view(f32)) & (np.arange(ROW_WORDS) < nv)
    assert isn[5, 0] and not isn[:5].any()
    assert (np.isnan(got.view(f32)) & (np.arange(ROW_WORDS) < nv) == isn).all()
    got, want = np.where(isn, 0, got), np.where(isn, 0, want)
    assert_rows_equal(got, want, nv)
    assert (want[0] == 0).all()
    if block == 1024:
        assert int(cnts[7, :, 0].astype(np.uint64).sum()) >= 1 << 32, "the count must have wrapped in this case"
