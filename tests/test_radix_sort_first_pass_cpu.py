"""radix_first_pass() (csrc/radix_sort.h), the contract a kernel that makes keys follows to leave the sort's first tile
histograms: tile count, keys per tile, digit width and mask for every key width. Host code only. No GPU."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    from sycl_points_amd import _lib

    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("n", [1, 2048, 2049, 10**6])
def test_radix_first_pass_tiles_digit_and_mask(L, n):
    for bits in range(1, 33):
        out4 = (C.c_uint * 4)()
        L.sp_internal_radix_first_pass(n, bits, out4)
        tiles, tile_keys, digit, mask = (int(v) for v in out4)
        assert tiles * tile_keys >= n > (tiles - 1) * tile_keys, (n, bits)
        assert digit in (8, 9), (n, bits)
        assert mask == 2 ** min(bits, digit) - 1, (n, bits)
        assert (digit == 9) == (-(-bits // 9) < -(-bits // 8)), (n, bits)  # 9-bit digits exactly where they save a pass
