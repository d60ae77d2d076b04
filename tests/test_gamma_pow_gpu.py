"""GPU: the step kernels' gamma pow for the three literal exponents, and the lemma behind their frame-1
shortcut, checked on the device over whole ranges of operand bit patterns (rtDiagGammaPow: one
grid-stride launch per sweep, a mismatch count and the first mismatching operand come back).

(a) pow_gamma<Y>(x) has the bits of the math mode's own pow(x, Y) for every one of the 2^32 operands --
    NaN results included -- for 2.2f, 0.454545f and 0.45454545f, in the devicelib and shipped modes
    (the modes whose pow is the device library's; pinned keeps its pow and is swept as the identity).
(b) for every stored value x of the safe set (bits <= 0x5C000000: +0 .. 2^57, or -0) the product
    pow(x, 2.2f) * 0.0f has the bits of +0 in all three modes, which is what lets frame number 1 leave
    FromGamma(old) out.  The two operands just outside the set are recorded, not asserted."""
import pytest

from clrt import _native as N

pytestmark = pytest.mark.gpu

MATHS = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}
SAFE_LAST = 0x5C000000   # 2^57
NEG_ZERO = 0x80000000


@pytest.mark.parametrize("exponent", list(N.GAMMA_EXPONENTS))
@pytest.mark.parametrize("math", ["devicelib", "shipped"])
def test_pow_gamma_equals_the_library_pow_everywhere(math, exponent):
    bad, first, _ = N.gamma_pow_check(MATHS[math], "pow", exponent, 0, 1 << 32)
    print(f"{math} {exponent}: {bad} mismatches" + (f", first at 0x{first:08x}" if bad else ""))
    assert bad == 0, f"first mismatch at x = 0x{first:08x}"


def test_pow_gamma_pinned_is_its_pow():
    # the fp64 pow is slow and pow_gamma is that call: the edges of every class, not the whole domain
    for first, count in ((0, 1 << 16), (0x3F7F0000, 1 << 17), (0x5BFF0000, 1 << 17), (0x7F7F0000, 1 << 17),
                         (0x80000000, 1 << 16), (0xBF7F0000, 1 << 17), (0xFF7F0000, 1 << 16)):
        count = min(count, (1 << 32) - first)
        for exponent in N.GAMMA_EXPONENTS:
            assert N.gamma_pow_check(N.MATH_PINNED, "pow", exponent, first, count)[0] == 0


def test_sweep_reports_mismatches():
    # the lemma does not hold for 1.0 .. (1 * 0 = +0 does; NaN does not): the sweep's own plumbing,
    # over +inf and the NaNs behind it, every one of which gives NaN * 0 = NaN
    bad, first, bits = N.gamma_pow_check(N.MATH_SHIPPED, "lemma", first=0x7F800000, count=1 << 12)
    assert (bad, first) == (1 << 12, 0x7F800000) and bits & 0x7FFFFFFF > 0x7F800000
    with pytest.raises(Exception):
        N.gamma_pow_check(N.MATH_SHIPPED, "pow", first=1, count=1 << 32)   # past the last pattern


@pytest.mark.parametrize("math", list(MATHS))
def test_frame_one_lemma_over_the_safe_set(math):
    m = MATHS[math]
    bad, first, at_zero = N.gamma_pow_check(m, "lemma", first=0, count=SAFE_LAST + 1)
    assert bad == 0, f"pow(x, 2.2f) * 0.0f is not +0 at x = 0x{first:08x}"
    assert at_zero == 0
    assert N.gamma_pow_check(m, "lemma", first=NEG_ZERO, count=1) == (0, None, 0)
    # just outside the set: recorded only (the next float above 2^57, the smallest negative denormal)
    for x in (SAFE_LAST + 1, NEG_ZERO + 1):
        bad, _, bits = N.gamma_pow_check(m, "lemma", first=x, count=1)
        print(f"{math}: pow(0x{x:08x}, 2.2f) * 0.0f = 0x{bits:08x} ({'+0' if not bad else 'not +0'})")
