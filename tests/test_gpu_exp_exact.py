"""The composites' exp (csrc/olsr_device.h: pinned_expf, pinned_expf2) returns the bits of the sequence it replaced
(pinned_expf_ref: rint, float -> int, multiply by 2^n) — rounding by magic constant, the scale from the bits of the rounded
sum, one fma for the last step; DESIGN.md section 5 has the three equivalences.  Swept on the GPU over EVERY float32 the
composites can hand it: -0 ... -90 (the clamp at -87 included) and +0 ... +88, plus the specials, in three forms: scalar,
packed with the argument in lane x and a different one in lane y, packed with the lanes swapped (a toolchain trap gives lane y
lane x's scale when the packed scale is written per component, which equal lanes would hide)."""
import pytest

from online_lang_splatting_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lo,hi", _abi.EXP_SWEEP_RANGES, ids=["minus0_to_minus90", "plus0_to_plus88"])
def test_every_consumed_argument_gives_the_reference_bits(hip, lo, hi):
    from online_lang_splatting_amd import _lib
    scalar, packed, swapped, first = _lib.exp_sweep(lo, hi - lo + 1)
    print(f"exp sweep [{lo:#010x}, {hi:#010x}]: {hi - lo + 1} patterns, mismatches scalar {scalar} packed {packed} "
          f"swapped {swapped}, first {first if first is None else hex(first)}")
    assert (scalar, packed, swapped, first) == (0, 0, 0, None)


@pytest.mark.parametrize("bits", _abi.EXP_SWEEP_SPECIALS, ids=[f"{b:#010x}" for b in _abi.EXP_SWEEP_SPECIALS])
def test_specials(hip, bits):
    from online_lang_splatting_amd import _lib
    got = _lib.exp_sweep(bits, 1)
    print(f"exp special {bits:#010x}: {got}")
    assert got == (0, 0, 0, None)


def test_argument_checks(hip):
    from online_lang_splatting_amd import _lib
    L = _lib.lib()
    import ctypes
    out = (ctypes.c_uint64 * 4)()
    assert L.olsr_debug_exp_sweep(0, 1, None) == _abi.OLSR_ERR_ARG
    assert L.olsr_debug_exp_sweep(0xFFFFFFFF, 2, out) == _abi.OLSR_ERR_ARG   # runs past the last pattern
    assert L.olsr_debug_exp_sweep(0xC1200000, 0, out) == _abi.OLSR_OK and list(out) == [0, 0, 0, 2**64 - 1]
