"""PointCloud2 ingestion without a GPU: the field resolution (sp_pc2_resolve_fields_host), the argument checks of sp_pc2_unpack,
sp_pc2_pack and sp_enhanced_reflectivity that return before any HIP call, the symbols, the compiler's resource report, and the
numpy restatement that tests/test_gpu_pointcloud2.py holds the device to, with its own pins.

The restatement is written from the formulas in include/sycl_points_amd.h: structured dtypes with explicit offsets and
itemsize = point_step for the records, one correctly rounded IEEE operation per step, and a plain sequential loop for the
reflectivity correction (float32, or float64 as the yardstick of the general case).

Tolerance of the general reflectivity case (used by the GPU test, checked here on the restatement itself). All summands of a
ring's sums are non-negative, so any order of c additions has relative error at most (c - 1) * 2^-24 to first order. The other
roundings behind one output are range_sq (3: two of its terms and the sum are rounded; counted 4), the two products / quotients
(2), the means (2), three per EMA step and scan (3 s), the final quotients and the sum (3): at most 16 + 3 s units. Hence, before
clamping, |value - f64| <= (c_max + 16 + 3 s) * 2^-24 * f64 with c_max the largest per-ring count and s the number of scans.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sycl_points_amd.h")
I8, U8, I16, U16, I32, U32, F32, F64 = range(1, 9)  # sensor_msgs/PointField
NP_OF = {U8: "u1", U16: "<u2", U32: "<u4", F32: "<f4", F64: "<f8"}
STAMP = (1_700_000_000, 250_000_000)  # the header stamp of every synthetic message
START_MS = float(STAMP[0]) * 1000.0 + float(STAMP[1]) * 1e-6


def header_constant(name):
    return int(re.search(rf"#define {name} (\d+)", open(HEADER).read()).group(1))


B = header_constant("SP_PC2_BLOCK_POINTS")  # records per workgroup
SIZES = (1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 7)

# name -> (point_step, [(field, offset, type)]): records that are no multiple of 16 bytes somewhere
LAYOUTS = {
    "a": (48, [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 16, F32), ("t", 20, U32), ("reflectivity", 24, U16),
               ("ring", 26, U16), ("ambient", 28, U16)]),  # Ouster
    "b": (22, [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 12, F32), ("ring", 16, U16), ("time", 18, F32)]),  # Velodyne
    "c": (26, [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 12, F32), ("flag0", 16, U8), ("flag1", 17, U8),
               ("timestamp", 18, F64)]),  # unaligned doubles, absolute Unix times
    "d": (33, [("x", 0, F64), ("y", 8, F64), ("z", 16, F64), ("rgba", 24, U32)]),  # (one pad byte at 32)
    "e": (48, [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 16, U16), ("t", 20, U32), ("rgb", 24, F32),
               ("ring", 28, U16), ("ambient", 30, U16)]),
}
# the reflectivity messages: layout (a), and a 19-byte record with a one-byte ring and an unaligned ambient
ER_LAYOUTS = {
    "u16": LAYOUTS["a"],
    "u8": (19, [("x", 0, F32), ("y", 4, F32), ("z", 8, F32), ("intensity", 12, F32), ("ring", 16, U8), ("ambient", 17, U16)]),
}


def record_dtype(layout):
    step, fields = layout
    return np.dtype({"names": [f[0] for f in fields], "formats": [NP_OF[f[2]] for f in fields], "offsets": [f[1] for f in fields],
                     "itemsize": step})


def lib():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib, C.CDLL(_lib.LIB_PATH)


def resolve(fields, point_step, rgb=True, intensity=True, reflectivity=True):
    """sp_pc2_resolve_fields_host -> (return code, layout)"""
    _lib, L = lib()
    nf = len(fields)
    names = (C.c_char_p * max(nf, 1))(*[f[0].encode() for f in fields])
    offsets = (C.c_uint32 * max(nf, 1))(*[f[1] for f in fields])
    types = (C.c_uint8 * max(nf, 1))(*[f[2] for f in fields])
    out = _lib.Pc2Layout()
    L.sp_pc2_resolve_fields_host.restype = C.c_int
    L.sp_pc2_resolve_fields_host.argtypes = _lib.SIGNATURES["sp_pc2_resolve_fields_host"][1]
    rc = L.sp_pc2_resolve_fields_host(names, offsets, types, nf, point_step, int(rgb), int(intensity), int(reflectivity), C.byref(out))
    return rc, out


# ------------------------------------------------------------------------------------------------ synthetic messages
COORD_SPECIALS = (0.0, -0.0, 1e-40, -3e-42, np.inf, -np.inf, np.nan)  # zero, denormals, infinities, NaN
COORD_SPECIALS_F64 = COORD_SPECIALS + (1e39, -1e39, 3.4e38, 1e-50)  # beyond float's range either way
TS_U32 = (0, 2 ** 24 + 1, 2 ** 32 - 1, 1_000_000, 99_999_999)
TS_F32 = (np.nan, np.inf, -np.inf, -0.25, 0.0, 0.05, 0.1)
TS_F64 = (np.nan, np.inf, -1.0, 0.0, -0.0, 0.05, float(STAMP[0]) + 0.35, float(STAMP[0]) - 5.0, float(STAMP[0]) + 0.251, 1e8)


def make_message(name, n, seed=7):
    """n records of layout `name` as a structured array (tobytes() is the message's data)"""
    layout = LAYOUTS[name]
    rs = np.random.RandomState(seed)
    rec = np.zeros(n, record_dtype(layout))
    types = {f[0]: f[2] for f in layout[1]}
    for k, axis in enumerate("xyz"):
        specials = COORD_SPECIALS_F64 if types[axis] == F64 else COORD_SPECIALS
        v = rs.uniform(-50, 50, n)
        for j, s in enumerate(specials):  # the specials of the three axes on different rows
            if 3 * j + k < n:
                v[3 * j + k] = s
        with np.errstate(over="ignore"):
            rec[axis] = v.astype(rec.dtype[axis])
    cyc = lambda vals, dt: np.array([vals[i % len(vals)] for i in range(n)], dt)  # noqa: E731
    for f, _, t in layout[1]:
        if f in ("intensity", "reflectivity", "ambient"):
            rec[f] = rs.uniform(0, 300, n).astype(np.float32) if t == F32 else rs.randint(0, 65536, n)
        elif f in ("rgb", "rgba"):
            rec[f] = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(rec.dtype[f])
        elif f == "ring":
            rec[f] = np.arange(n) % 128
        elif f in ("t", "time", "timestamp"):
            rec[f] = cyc({U32: TS_U32, F32: TS_F32, F64: TS_F64}[t], rec.dtype[f])
        elif f.startswith("flag"):
            rec[f] = rs.randint(0, 256, n)
    if "rgb" in rec.dtype.names and n > 2:  # bytes 0 and 255 in every channel
        rec["rgb"][:2] = np.array([0x00FF00FF, 0xFF00FF00], np.uint32).view(np.float32)
    if "rgba" in rec.dtype.names and n > 2:
        rec["rgba"][:2] = (0x00FF00FF, 0xFF00FF00)
    return rec


# ------------------------------------------------------------------------------------------------ the restatement
def restate_unpack(data, n, L):
    """sp_pc2_unpack on the first n records of `data` (bytes) with the resolved layout L:
    (points, rgb or None, intensities or None, timestamps or None, max offset or None)"""
    def col(offset, fmt):
        dt = np.dtype({"names": ["v"], "formats": [fmt], "offsets": [offset], "itemsize": L.point_step})
        return np.frombuffer(data, dt, count=n)["v"]

    points = np.ones((n, 4), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, off in enumerate((L.x_offset, L.y_offset, L.z_offset)):
            points[:, k] = col(off, NP_OF[L.xyz_type]).astype(np.float32)  # (float64: round to nearest, inf beyond the range)
    rgb = inten = ts = mx = None
    if L.rgb_offset >= 0:
        c = col(L.rgb_offset, "<u4")
        rgb = np.stack([((c >> (8 * k)) & 0xFF).astype(np.float32) / np.float32(255.0) for k in range(4)], 1)
    if L.intensity_offset >= 0:
        inten = col(L.intensity_offset, NP_OF[L.intensity_type]).astype(np.float32)
    if L.timestamp_offset >= 0:
        raw = col(L.timestamp_offset, NP_OF[L.timestamp_type])
        with np.errstate(over="ignore", invalid="ignore"):
            if L.timestamp_type == U32:
                ts = raw.astype(np.float32) * np.float32(1e-6)
                off = ts.astype(np.float64)
            elif L.timestamp_type == F32:
                r = raw.astype(np.float64)
                off = np.where(np.isfinite(r) & (r > 0.0), r * 1e3, 0.0)
                ts = off.astype(np.float32)
            else:
                off = np.where(raw > 1e8, raw * 1e3 - L.start_time_ms, raw * 1e3)
                off = np.where(off < 0.0, 0.0, off)
                off = np.where(np.isfinite(raw) & (raw >= 0.0), off, 0.0)
                ts = off.astype(np.float32)
        mx = float(off.max())
        mx = mx if mx > 0.0 else 0.0  # std::max(0.0, -0.0) keeps +0.0
    return points, rgb, inten, ts, mx


def pack_dtype(has_rgb, has_int, has_ts):
    names, formats = ["p"], [("<f4", 4)]
    for present, name, fmt in ((has_rgb, "rgb", ("u1", 4)), (has_int, "intensity", "<f4"), (has_ts, "timestamp", "<f8")):
        if present:
            names.append(name)
            formats.append(fmt)
    offsets, at = [], 0
    for f in formats:
        offsets.append(at)
        at += np.dtype(f).itemsize
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": at})


def restate_pack(points, rgb, inten, ts, start_ms):
    """sp_pc2_pack: the records as bytes. NaN in rgb gives 0: clamp is fminf(fmaxf(c, 0), 1) and fmaxf(NaN, 0) = 0."""
    dt = pack_dtype(rgb is not None, inten is not None, ts is not None)
    rec = np.zeros(len(points), dt)
    rec["p"] = points
    if rgb is not None:
        rec["rgb"] = (np.fmin(np.fmax(rgb, np.float32(0)), np.float32(1)) * np.float32(255.0)).astype(np.uint8)  # truncates
    if inten is not None:
        rec["intensity"] = inten
    if ts is not None:
        rec["timestamp"] = (start_ms + ts.astype(np.float64)) * 1e-3
    return rec.tobytes()


def new_state(ft=np.float32):
    return [np.zeros(256, ft), np.zeros(256, ft), np.zeros(256, bool)]


def restate_reflectivity(points, inten, ring, ambient, state, alpha, clip_max, ft=np.float32):
    """EnhancedReflectivityCorrector::apply as a sequential loop in `ft`; updates `state` in place and returns
    (clamped intensities, the values before clamping, per-ring counts)"""
    n = len(points)
    F = ft
    eps = F(np.float32(1e-6))
    ref, amb = np.zeros(n, ft), np.zeros(n, ft)
    sum_ref, sum_amb, count = np.zeros(256, ft), np.zeros(256, ft), np.zeros(256, np.int64)
    for i in range(n):
        x, y, z = F(points[i, 0]), F(points[i, 1]), F(points[i, 2])
        range_sq = x * x + y * y + z * z
        if range_sq < eps:
            continue
        ref[i] = F(inten[i]) * range_sq
        amb[i] = F(float(ambient[i])) / range_sq
        r = int(ring[i])
        if r < 256:
            sum_ref[r] += ref[i]
            sum_amb[r] += amb[i]
            count[r] += 1
    mean_ref, mean_amb, init = state
    a = F(np.float32(alpha))
    for r in range(256):
        if count[r] > 0:
            c = F(float(count[r]))
            new_ref, new_amb = sum_ref[r] / c, sum_amb[r] / c
            if not init[r]:
                mean_ref[r], mean_amb[r], init[r] = new_ref, new_amb, True
            else:
                mean_ref[r] = a * new_ref + (F(1.0) - a) * mean_ref[r]
                mean_amb[r] = a * new_amb + (F(1.0) - a) * mean_amb[r]
    raw = np.zeros(n, ft)
    for i in range(n):
        r = int(ring[i])
        if r >= 256:
            continue
        u, v = ref[i], amb[i]
        if mean_ref[r] > 0:
            u = u / mean_ref[r]
        if mean_amb[r] > 0:
            v = v / mean_amb[r]
        raw[i] = u + v
    clip = F(np.float32(clip_max))
    out = np.where(raw < 0, F(0), np.where(clip < raw, clip, raw)).astype(ft)
    return out, raw, count


def reflectivity_message(kind, points, inten, ring, ambient):
    rec = np.zeros(len(points), record_dtype(ER_LAYOUTS[kind]))
    rec["x"], rec["y"], rec["z"] = points[:, 0], points[:, 1], points[:, 2]
    rec["intensity"], rec["ring"], rec["ambient"] = inten, ring, ambient
    if "reflectivity" in rec.dtype.names:
        rec["reflectivity"] = 7
    return rec


def general_scan(kind, scan):
    """8192 random points spread evenly over 16 rings, with rows that ride along inside that total: rings that are out of range
    (300; the one-byte ring field cannot hold it and gets the otherwise unused ring 200) and points at the sensor"""
    n = 8192
    rs = np.random.RandomState(100 + scan)
    points = np.ones((n, 4), np.float32)
    points[:, :3] = rs.uniform(-20, 20, (n, 3))
    ring = (np.arange(n) % 16).astype(np.int64)
    odd = rs.permutation(n)
    ring[odd[:40]] = 300 if kind == "u16" else 200
    points[odd[40:80], :3] = rs.uniform(-3e-4, 3e-4, (40, 3))  # range_sq < 1e-6
    inten = rs.uniform(0, 200, n).astype(np.float32)
    ambient = rs.randint(0, 5000, n)
    return points, inten, ring, ambient


def exact_scan(scan):
    """Inputs for which every sum is exact in any order: one coordinate from {1, 2, 4} (range_sq 1, 4 or 16), integer intensities
    <= 255 (ref <= 4080: a ring's sum of <= 512 of them stays below 2^24), ambient = 16 k with k < 1000 (amb = 16 k / range_sq is an
    integer <= 16000: the sum stays below 2^24 too; an unrestricted multiple of 16 could pass it). 5003 points on 12 rings, at most
    417 per ring; the third scan leaves ring 5 out. Rows with ring 300 and rows at the origin ride along."""
    n = 5003
    rs = np.random.RandomState(200 + scan)
    points = np.zeros((n, 4), np.float32)
    points[:, 3] = 1.0
    points[np.arange(n), rs.randint(0, 3, n)] = rs.choice([1.0, 2.0, 4.0], n)
    ring = (np.arange(n) % 12).astype(np.int64)
    if scan == 2:
        ring[ring == 5] = 300
    odd = rs.permutation(n)
    ring[odd[:30]] = 300
    points[odd[30:60], :3] = 0.0
    inten = rs.randint(0, 256, n).astype(np.float32)
    ambient = 16 * rs.randint(0, 1000, n)
    return points, inten, ring, ambient


def reflectivity_bound(c_max, scans):
    return (c_max + 16 + 3 * scans) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the tests
def test_symbols_and_abi():
    _lib, L = lib()
    for s in ("sp_pc2_resolve_fields_host", "sp_pc2_unpack_workspace_bytes", "sp_pc2_unpack", "sp_pc2_pack_point_step", "sp_pc2_pack",
              "sp_enhanced_reflectivity_workspace_bytes", "sp_enhanced_reflectivity"):
        assert hasattr(L, s) and s in _lib.SIGNATURES
    assert _lib.lib().sp_abi_version() == 7
    assert (_lib.PC2_BLOCK_POINTS, _lib.PC2_MAX_POINT_STEP, _lib.ER_MAX_RINGS) == tuple(
        header_constant(k) for k in ("SP_PC2_BLOCK_POINTS", "SP_PC2_MAX_POINT_STEP", "SP_ER_MAX_RINGS"))
    assert C.sizeof(_lib.Pc2Layout) == 40 and _lib.Pc2Layout.start_time_ms.offset == 32
    assert [_lib.lib().sp_pc2_pack_point_step(*f) for f in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))] == [16, 20, 20, 24, 32]


def test_kernels_use_no_scratch():
    lib()
    rows = open(os.path.join(ROOT, "sycl_points_amd", "lib", "pointcloud2.resources.txt")).read().splitlines()
    names = [k for k in ("pc2_unpack_kernel", "pc2_max_kernel", "pc2_pack_kernel", "er_partials_kernel", "er_update_kernel", "er_apply_kernel")
             if any(k in r for r in rows)]
    assert len(names) == 6 and len(rows) == 6, rows
    for r in rows:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", r).group(1)) == 0, r
        assert int(re.search(r"VGPRs Spill: (\d+)", r).group(1)) == 0, r


XYZ = [("x", 0, F32), ("y", 4, F32), ("z", 8, F32)]


@pytest.mark.parametrize("alias", ["t", "time", "timestamp", "offset_time"])
def test_timestamp_aliases(alias):
    for t in (F32, F64, U32):
        rc, L = resolve(XYZ + [(alias, 12, t)], 20)
        assert rc == 0 and (L.timestamp_offset, L.timestamp_type) == (12, t)
    rc, L = resolve(XYZ + [(alias, 12, U16)], 20)  # a type the reference does not convert: dropped
    assert rc == 0 and (L.timestamp_offset, L.timestamp_type) == (-1, 0)


def test_name_table_and_switches():
    rc, L = resolve(XYZ + [("not_a_field", 12, F32)], 16)
    assert rc == 0 and (L.point_step, L.x_offset, L.y_offset, L.z_offset, L.xyz_type) == (16, 0, 4, 8, F32)
    assert (L.rgb_offset, L.intensity_offset, L.timestamp_offset, L.start_time_ms) == (-1, -1, -1, 0.0)
    for name in ("rgb", "rgba"):
        for t in (F32, U32):
            rc, L = resolve(XYZ + [(name, 12, t)], 16)
            assert rc == 0 and (L.rgb_offset, L.rgb_type) == (12, t)
        assert resolve(XYZ + [(name, 12, U32)], 16, rgb=False)[1].rgb_offset == -1
        rc, L = resolve(XYZ + [(name, 12, F64)], 20)  # unsupported: dropped, no error
        assert rc == 0 and (L.rgb_offset, L.rgb_type) == (-1, 0)
    both = XYZ + [("intensity", 12, F32), ("reflectivity", 16, U16)]
    L = resolve(both, 18)[1]
    assert (L.intensity_offset, L.intensity_type) == (16, U16)  # reflectivity preferred
    L = resolve(both, 18, reflectivity=False)[1]
    assert (L.intensity_offset, L.intensity_type) == (12, F32)  # the switch is off
    L = resolve(XYZ + [("intensity", 12, F32), ("reflectivity", 16, U8)], 18)[1]
    assert (L.intensity_offset, L.intensity_type) == (12, F32)  # the wrong type does not take over
    L = resolve(XYZ + [("reflectivity", 12, U16)], 14)[1]
    assert (L.intensity_offset, L.intensity_type) == (12, U16)
    assert resolve(both, 18, intensity=False)[1].intensity_offset == -1
    L = resolve(XYZ + [("intensity", 12, U16)], 14)[1]
    assert (L.intensity_offset, L.intensity_type) == (12, U16)
    rc, L = resolve(XYZ + [("intensity", 12, U8)], 14)  # unsupported: dropped
    assert rc == 0 and (L.intensity_offset, L.intensity_type) == (-1, 0)
    d = [("x", 0, F64), ("y", 8, F64), ("z", 16, F64)]
    rc, L = resolve(d, 24)
    assert rc == 0 and (L.xyz_type, L.z_offset) == (F64, 16)
    for name, (step, fields) in LAYOUTS.items():
        assert resolve(fields, step)[0] == 0, name


def test_resolution_errors():
    _lib, _ = lib()
    assert resolve([("x", 0, F32), ("z", 8, F32)], 12)[0] == _lib.SP_ERR_RUNTIME  # no y
    assert resolve([("x", 0, F32), ("y", 4, F64), ("z", 12, F32)], 16)[0] == _lib.SP_ERR_RUNTIME  # mixed types
    assert resolve([("x", 0, U32), ("y", 4, U32), ("z", 8, U32)], 12)[0] == _lib.SP_ERR_RUNTIME
    assert resolve([], 12)[0] == _lib.SP_ERR_RUNTIME
    assert resolve(XYZ, 11)[0] == _lib.SP_ERR_INVALID_ARGUMENT  # z runs past the record
    assert resolve(XYZ + [("timestamp", 12, F64)], 19)[0] == _lib.SP_ERR_INVALID_ARGUMENT
    assert resolve(XYZ + [("timestamp", 12, F64)], 20)[0] == 0
    assert resolve(XYZ + [("intensity", 15, U16)], 16)[0] == _lib.SP_ERR_INVALID_ARGUMENT
    assert resolve(XYZ + [("intensity", 15, U8)], 16)[0] == 0  # a dropped field is not measured
    assert resolve(XYZ, 0)[0] == _lib.SP_ERR_INVALID_ARGUMENT


def test_argument_checks_return_before_any_hip_call():
    """every pointer is a made-up address: an entry point that touched the device with it, or got past its checks, would fault"""
    _lib, _ = lib()
    L = _lib.lib()
    INV = _lib.SP_ERR_INVALID_ARGUMENT
    ok = resolve(LAYOUTS["a"][1], 48)[1]
    P = lambda a: C.c_void_p(a)  # noqa: E731
    good = dict(data=P(0x1000), nbytes=48 * 10, n=10, lay=C.byref(ok), pts=P(0x2000), rgb=None, inten=P(0x3000), ts=P(0x4000), mx=P(0x5000), ws=P(0x6000))
    call = lambda **kw: L.sp_pc2_unpack(*[{**good, **kw}[k] for k in ("data", "nbytes", "n", "lay", "pts", "rgb", "inten", "ts", "mx", "ws")], None)  # noqa: E731
    assert call(n=0) == 0  # nothing enqueued
    assert call(lay=None) == INV
    assert call(data=None) == INV and call(data=P(0x1008)) == INV  # null, not 16-byte aligned
    assert call(nbytes=48 * 10 - 1) == INV  # n * point_step > data_bytes
    assert call(n=2 ** 32, nbytes=2 ** 40) == INV
    assert call(pts=None) == INV and call(inten=None) == INV and call(ts=None) == INV and call(mx=None) == INV
    assert call(ws=None) == INV and call(ws=P(0x6008)) == INV  # a time stamp field needs the workspace
    assert [L.sp_pc2_unpack_workspace_bytes(n) for n in (0, 1, B, B + 1)] == [0, 8, 8, 16]
    for field, value in (("point_step", 0), ("point_step", _lib.PC2_MAX_POINT_STEP + 1), ("xyz_type", U32), ("intensity_type", U8),
                         ("timestamp_type", U16), ("timestamp_offset", 46), ("z_offset", 45), ("start_time_ms", float("nan"))):
        bad = _lib.Pc2Layout.from_buffer_copy(ok)
        setattr(bad, field, value)
        assert call(lay=C.byref(bad), nbytes=2 ** 20) == INV, field
    with_rgb = resolve(LAYOUTS["e"][1], 48)[1]
    assert call(lay=C.byref(with_rgb), rgb=None) == INV
    # pack
    assert L.sp_pc2_pack(P(0x1000), None, None, None, 0, 0.0, P(0x2000), None) == 0
    assert L.sp_pc2_pack(None, None, None, None, 5, 0.0, P(0x2000), None) == INV
    assert L.sp_pc2_pack(P(0x1000), None, None, None, 5, 0.0, None, None) == INV
    assert L.sp_pc2_pack(P(0x1000), None, None, None, 5, 0.0, P(0x2004), None) == INV
    assert L.sp_pc2_pack(P(0x1000), None, None, None, 2 ** 32, 0.0, P(0x2000), None) == INV
    # reflectivity
    er = dict(pts=P(0x1000), inten=P(0x2000), n=10, data=P(0x3000), step=48, ring=26, u8=0, amb=28, state=P(0x4000), ws=P(0x5000))
    ecall = lambda **kw: L.sp_enhanced_reflectivity(*[{**er, **kw}[k] for k in ("pts", "inten", "n", "data", "step", "ring", "u8", "amb", "state")],  # noqa: E731
                                                    0.5, 5.0, {**er, **kw}["ws"], None)
    assert ecall(n=0) == 0
    for k in ("pts", "inten", "data", "state", "ws"):
        assert ecall(**{k: None}) == INV, k
    assert ecall(data=P(0x3004)) == INV and ecall(ws=P(0x5008)) == INV
    assert ecall(step=0) == INV and ecall(step=_lib.PC2_MAX_POINT_STEP + 1) == INV and ecall(n=2 ** 32) == INV
    assert ecall(ring=47) == INV and ecall(ring=-1) == INV and ecall(amb=47) == INV and ecall(amb=-1) == INV
    assert ecall(ring=47, u8=1, n=0) == 0
    assert L.sp_enhanced_reflectivity_workspace_bytes(0) == 0
    for n in (1, 512, 513, 131072, 2048 * 512, 2048 * 512 + 1, 10 ** 8):  # a fixed partition: a function of n alone, never more than 2048 spans
        w = L.sp_enhanced_reflectivity_workspace_bytes(n)
        assert w % (3 * 256 * 4) == 0 and 1 <= w // (3 * 256 * 4) <= 2048


def test_restatement_pins_unpack():
    """hand-computed values for the formulas the GPU test relies on"""
    L = resolve(LAYOUTS["a"][1], 48)[1]
    rec = make_message("a", len(TS_U32))
    rec["reflectivity"][:2] = (0, 65535)
    pts, rgb, inten, ts, mx = restate_unpack(rec.tobytes(), len(rec), L)
    assert rgb is None and inten[0] == 0.0 and inten[1] == 65535.0  # reflectivity took over
    assert np.array_equal(pts[:, 3], np.ones(len(rec), np.float32))
    assert ts[0] == 0.0 and ts[1] == np.float32(2 ** 24) * np.float32(1e-6)  # 2^24 + 1 rounds to even
    assert ts[2] == np.float32(2 ** 32) * np.float32(1e-6) and mx == float(ts[2])
    L = resolve(LAYOUTS["b"][1], 22)[1]
    pts, _, _, ts, mx = restate_unpack(make_message("b", len(TS_F32)).tobytes(), len(TS_F32), L)
    assert list(ts[:5]) == [0, 0, 0, 0, 0] and ts[5] == np.float32(float(np.float32(0.05)) * 1e3) and mx == float(np.float32(0.1)) * 1e3
    assert pts[0, 0] == 0 and np.signbit(pts[3, 0]) and pts[6, 0].view(np.uint32) == np.float32(1e-40).view(np.uint32) != 0  # specials of x: rows 0, 3, 6, ...
    L = resolve(LAYOUTS["c"][1], 26)[1]
    L.start_time_ms = START_MS
    _, _, _, ts, mx = restate_unpack(make_message("c", len(TS_F64)).tobytes(), len(TS_F64), L)
    assert list(ts[:4]) == [0, 0, 0, 0] and np.signbit(ts[4]) and ts[5] == np.float32(50.0)
    assert ts[6] == np.float32((float(STAMP[0]) + 0.35) * 1e3 - START_MS) and 99.9 < ts[6] < 100.1  # after the stamp
    assert ts[7] == 0.0 and 0.99 < ts[8] < 1.01  # before the stamp; 1 ms after it (a double of 1.7e9 s resolves 2.4e-4 ms)
    assert ts[9] == np.float32(1e11) and mx == 1e11  # exactly 1e8 s is still a relative offset
    assert restate_unpack(make_message("c", 5).tobytes(), 5, L)[4] == 0.0 and not np.signbit(restate_unpack(make_message("c", 5).tobytes(), 5, L)[4])
    L = resolve(LAYOUTS["d"][1], 33)[1]
    pts, rgb, _, ts, _ = restate_unpack(make_message("d", 40).tobytes(), 40, L)
    assert ts is None and pts[7 * 3, 0] == np.inf and pts[8 * 3 + 1, 1] == -np.inf and pts[9 * 3, 0] == np.float32(3.4e38) and pts[10 * 3, 0] == 0.0
    assert list(rgb[0]) == [1.0, 0.0, 1.0, 0.0] and list(rgb[1]) == [0.0, 1.0, 0.0, 1.0]
    assert rgb[2, 0] == np.float32(float(make_message("d", 40)["rgba"][2] & 0xFF)) / np.float32(255)


def test_restatement_pins_pack():
    p = np.array([[1, 2, 3, 1]], np.float32)
    rgb = np.array([[-0.5, 0.0, 0.999, 1.0], [1.5, np.nan, 0.5, 1.0 / 255.0]], np.float32)
    out = np.frombuffer(restate_pack(np.repeat(p, 2, 0), rgb, None, None, 0.0), pack_dtype(True, False, False))
    assert out["rgb"].tolist() == [[0, 0, 254, 255], [255, 0, 127, 1]]  # clamped, truncated, NaN -> 0
    out = np.frombuffer(restate_pack(p, None, np.float32([7.5]), np.float32([250.0]), START_MS), pack_dtype(False, True, True))
    assert out.dtype.itemsize == 28 and out["intensity"][0] == 7.5 and out["timestamp"][0] == (START_MS + 250.0) * 1e-3
    assert len(restate_pack(p, rgb[:1], np.float32([1]), np.float32([1]), 0.0)) == 32


def test_restatement_reflectivity_and_its_tolerance():
    """the sequential float32 restatement satisfies the GPU test's bound against float64 on the GPU test's inputs, with room to
    spare, and a ring that loses one of its ~512 points does not: the bound is safe for a correct sum and tight enough to see a
    dropped point"""
    for kind in ("u16", "u8"):
        s32, s64 = new_state(np.float32), new_state(np.float64)
        for scan in range(3):
            pts, inten, ring, amb = general_scan(kind, scan)
            _, raw32, count = restate_reflectivity(pts, inten, ring, amb, s32, 0.5, 1e30)
            _, raw64, _ = restate_reflectivity(pts, inten, ring, amb, s64, 0.5, 1e30, np.float64)
            bound = reflectivity_bound(int(count.max()), scan + 1)
            assert 500 <= count.max() <= 512 and (count > 0).sum() == (16 if kind == "u16" else 17)
            assert np.all(raw64 >= 0) and (raw64 == 0).sum() >= 40
            rel = np.abs(raw32.astype(np.float64) - raw64)[raw64 > 0] / raw64[raw64 > 0]
            print(f"[{kind} scan {scan}] restatement: max relative error {rel.max():.3e}, bound {bound:.3e}")
            assert rel.max() <= bound and np.array_equal(raw32 == 0, raw64 == 0)
        # one dropped point: ring 3 of a fresh first scan sums one point less
        pts, inten, ring, amb = general_scan(kind, 0)
        full = restate_reflectivity(pts, inten, ring, amb, new_state(np.float64), 0.5, 1e30, np.float64)[1]
        ring2 = ring.copy()
        victim = np.flatnonzero((ring == 3) & (np.abs(pts[:, :3]).max(1) > 1))[0]
        ring2[victim] = 400 if kind == "u16" else 201
        less = restate_reflectivity(pts, inten, ring2, amb, new_state(np.float64), 0.5, 1e30, np.float64)[1]
        on3 = (ring2 == 3) & (full > 0)
        assert (np.abs(less[on3] - full[on3]) / full[on3]).max() > 10 * reflectivity_bound(512, 1)


def test_restatement_reflectivity_exact_inputs_are_order_independent():
    """the exact case's claim: summed backwards the restatement gives the same bits, scan after scan"""
    fwd, bwd = new_state(), new_state()
    for scan in range(3):
        pts, inten, ring, amb = exact_scan(scan)
        a = restate_reflectivity(pts, inten, ring, amb, fwd, 0.5, 5.0)
        b = restate_reflectivity(pts[::-1], inten[::-1], ring[::-1], amb[::-1], bwd, 0.5, 5.0)
        assert np.array_equal(a[0].view(np.uint32), b[0][::-1].view(np.uint32)) and a[2].max() <= 512
        assert (a[0] == 5.0).any() and (a[0] == 0.0).any() and ((a[0] > 0) & (a[0] < 5.0)).any()
        for x, y in zip(fwd, bwd):
            assert np.array_equal(x, y)
    assert not fwd[2][12:].any() and fwd[2][:12].all()
