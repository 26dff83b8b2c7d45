"""Known answers for the Rust arithmetic tools/rsinterp has to reproduce, and for its panics.  CPU only, no reference tree needed.

tools/rsinterp executes the reference's Rust text to make the fixtures every bit-exact test here is held to, so a construct it reads
differently from rustc moves all of them together.  PROBES is a table of one-line expressions with the value rustc gives.  NO expectation
was read off the interpreter: each comes from the Rust Reference or the std documentation (the section is named in the row), or is
worked by hand from IEEE-754 binary32 / binary64 (24 / 53 significant bits, round to nearest, ties to even; the working is in the row).
Float results are compared as bit patterns (`to_bits()`), so signed zeros and the last place count.

The second half pins the interpreter's panics: the reference-unit-test cases (test_reference_unit_tests.py) mean something only if a
failed assertion, an `unwrap` of nothing, an index past the end or a division by zero raises RustPanic instead of passing quietly.
"""
import pytest

import rs_harness  # noqa: F401  (puts tools/ on the path)
from rsinterp import Interp, RustPanic

REF_CAST = "Rust Reference, Operator expressions, 'Numeric cast'"
REF_LIT = "Rust Reference, Tokens, 'String literals' / 'Byte string literals'"
REF_PREC = "Rust Reference, Expressions, 'Expression precedence'"
REF_ARITH = "Rust Reference, Operator expressions, 'Arithmetic and logical binary operators'"
REF_NEG = "Rust Reference, Operator expressions, 'Negation operators'"
IEEE = "IEEE-754 round to nearest, ties to even"

PROBES = [
    # ---- float -> int `as`: saturating, NaN -> 0, truncation toward zero
    ("300.0f32 as u8", "u8", 255, REF_CAST + ": saturates at the type's maximum"),
    ("-1.5f32 as u8", "u8", 0, REF_CAST + ": saturates at the type's minimum"),
    ("-1.9f32 as i32", "i32", -1, REF_CAST + ": rounds toward zero"),
    ("1.9f64 as i32", "i32", 1, REF_CAST + ": rounds toward zero"),
    ("0.99999f32 as i32", "i32", 0, REF_CAST + ": rounds toward zero"),
    ("-0.99999f64 as i64", "i64", 0, REF_CAST + ": rounds toward zero"),
    ("f32::NAN as i32", "i32", 0, REF_CAST + ": NaN gives 0"),
    ("f64::NAN as u8", "u8", 0, REF_CAST + ": NaN gives 0"),
    ("f32::INFINITY as i32", "i32", 2147483647, REF_CAST),
    ("f32::NEG_INFINITY as i32", "i32", -2147483648, REF_CAST),
    ("f64::NEG_INFINITY as u32", "u32", 0, REF_CAST),
    ("1e10f32 as i16", "i16", 32767, REF_CAST),
    ("-129.0f32 as i8", "i8", -128, REF_CAST),
    ("2147483648.0f64 as i32", "i32", 2147483647, REF_CAST + ": 2^31 is one past i32::MAX"),
    ("4294967296.0f64 as u32", "u32", 4294967295, REF_CAST),
    ("-2147483649.0f64 as i32", "i32", -2147483648, REF_CAST),
    # ---- int -> int `as`: truncate, sign-extend from a signed source, zero-extend from an unsigned one
    ("300i32 as u8", "u8", 44, REF_CAST + ": 300 mod 256"),
    ("-1i32 as u8", "u8", 255, REF_CAST),
    ("-1i8 as u32", "u32", 4294967295, REF_CAST + ": sign-extends"),
    ("200u8 as i8", "i8", -56, REF_CAST + ": same bits, 200 - 256"),
    ("200u8 as i8 as i32", "i32", -56, REF_CAST),
    ("255u8 as i16", "i16", 255, REF_CAST + ": zero-extends"),
    ("0x1_2345_6789u64 as u32", "u32", 0x23456789, REF_CAST),
    ("-1i64 as u16", "u16", 65535, REF_CAST),
    ("0x8000u16 as i16", "i16", -32768, REF_CAST),
    ("-128i8 as i64", "i64", -128, REF_CAST),
    ("true as i32", "i32", 1, REF_CAST + ": bool to integer"),
    ("'A' as u32", "u32", 65, REF_CAST + ": char to integer"),
    # ---- int -> f32 at the ties (f32 holds 24 significant bits)
    ("(16777217i32 as f32).to_bits()", "u32", 0x4B800000, IEEE + ": 2^24+1 lies between 2^24 and 2^24+2; 2^24 has the even significand"),
    ("(16777219i32 as f32).to_bits()", "u32", 0x4B800002, IEEE + ": 2^24+3 lies between 2^24+2 (significand 2^23+1, odd) and 2^24+4 (even)"),
    ("(-16777217i32 as f32).to_bits()", "u32", 0xCB800000, IEEE + ": the mirror image of 2^24+1"),
    ("(33554434i64 as f32).to_bits()", "u32", 0x4C000000, IEEE + ": 2^25+2, spacing 4: tie between 2^25 (even) and 2^25+4"),
    ("(33554438i64 as f32).to_bits()", "u32", 0x4C000002, IEEE + ": 2^25+6: tie between 2^25+4 (odd) and 2^25+8 (even)"),
    ("(4294967295u32 as f32).to_bits()", "u32", 0x4F800000, IEEE + ": 2^32-1, spacing 256 below 2^32: nearest is 2^32"),
    ("(4294967167u32 as f32).to_bits()", "u32", 0x4F7FFFFF, IEEE + ": 2^32-129 is 127 from 2^32-256 and 129 from 2^32"),
    ("(4294967168u32 as f32).to_bits()", "u32", 0x4F800000, IEEE + ": 2^32-128: tie; 2^32-256 has significand 0xFFFFFF (odd), 2^32 is even"),
    ("(i64::MAX as f32).to_bits()", "u32", 0x5F000000, IEEE + ": 2^63-1 rounds to 2^63"),
    ("(i32::MIN as f32).to_bits()", "u32", 0xCF000000, "-2^31 is representable"),
    ("(9007199254740993i64 as f32).to_bits()", "u32", 0x5A000000, IEEE + ": 2^53+1, spacing 2^30: rounds to 2^53"),
    ("(18014399583223809i64 as f32).to_bits()", "u32", 0x5A800001,
     IEEE + ": 2^54+2^30+1 is just above the midpoint of 2^54 and 2^54+2^31, so it rounds UP; a conversion through f64 first "
     "(spacing 4 there) would drop the +1, land on the tie and round down to 0x5A800000"),
    ("(16777217i32 as f64) as i32", "i32", 16777217, "f64 holds 53 bits: exact"),
    # ---- f64 -> f32
    ("(0.1f64 as f32).to_bits()", "u32", 0x3DCCCCCD, IEEE + ": 0.1 = 0x1.999999999999Ap-4; 24 bits: 0x1.99999Ap-4"),
    ("(1.0000000596046448f64 as f32).to_bits()", "u32", 0x3F800000, IEEE + ": 1+2^-24 is the tie between 1 (even) and 1+2^-23"),
    ("(1.0000001788139343f64 as f32).to_bits()", "u32", 0x3F800002, IEEE + ": 1+3*2^-24 is the tie between 1+2^-23 (odd) and 1+2^-22 (even)"),
    ("(1e40f64 as f32).to_bits()", "u32", 0x7F800000, REF_CAST + ": beyond f32::MAX gives infinity"),
    ("(-1e40f64 as f32).to_bits()", "u32", 0xFF800000, REF_CAST),
    ("(1e-46f64 as f32).to_bits()", "u32", 0x00000000, IEEE + ": below half of the smallest subnormal 2^-149 = 1.4e-45"),
    ("(1e-45f64 as f32).to_bits()", "u32", 0x00000001, IEEE + ": above half of 2^-149 (7.0e-46), below 1.5 * 2^-149"),
    ("(-0.0f64 as f32).to_bits()", "u32", 0x80000000, "the sign of zero is kept"),
    ("(1.5f32 as f64).to_bits()", "u64", 0x3FF8000000000000, "f32 -> f64 is exact"),
    # ---- one rounding per f32 operation
    ("(16777216.0f32 + 1.0f32).to_bits()", "u32", 0x4B800000, IEEE + ": 2^24+1 is a tie, 2^24 is even"),
    ("(16777216.0f32 + 1.0f32 + 1.0f32).to_bits()", "u32", 0x4B800000, "each + rounds: (2^24 + 1) is 2^24 again, twice; summed in f64 it would be 2^24+2"),
    ("(0.1f32 + 0.2f32).to_bits()", "u32", 0x3E99999A,
     IEEE + ": 0.1f32 = 0xCCCCCD*2^-27, 0.2f32 = 0xCCCCCD*2^-26, sum = 40265319*2^-27 (26 bits); /4 = 10066329.75 -> 10066330 = 0x99999A"),
    ("(1.0f32 / 3.0f32).to_bits()", "u32", 0x3EAAAAAB, IEEE + ": 1/3 = 0x1.555555(5...)p-2, the 25th bit is 1 with more behind: up"),
    ("(2.0f32).sqrt().to_bits()", "u32", 0x3FB504F3, "sqrt is correctly rounded (IEEE-754): sqrt 2 = 0x1.6A09E667F...p0 -> 0x1.6A09E6p0"),
    ("(2.0f64).sqrt().to_bits()", "u64", 0x3FF6A09E667F3BCD, "sqrt is correctly rounded: the well-known f64 SQRT_2"),
    ("(3.0e38f32 + 3.0e38f32).to_bits()", "u32", 0x7F800000, "overflow gives infinity"),
    ("(f32::MAX * 2.0f32).to_bits()", "u32", 0x7F800000, "overflow gives infinity"),
    ("(f32::MIN_POSITIVE / 2.0f32).to_bits()", "u32", 0x00400000, "2^-127 is subnormal: significand 2^22"),
    ("(f32::MIN_POSITIVE * f32::EPSILON).to_bits()", "u32", 0x00000001, "2^-126 * 2^-23 = 2^-149, the smallest subnormal"),
    ("(f32::MIN_POSITIVE * f32::EPSILON * 0.5f32).to_bits()", "u32", 0x00000000, IEEE + ": 2^-150 is the tie between 0 (even) and 2^-149"),
    ("(f32::MIN_POSITIVE * f32::EPSILON * 0.75f32).to_bits()", "u32", 0x00000001, IEEE + ": 0.75 * 2^-149 is nearer 2^-149"),
    # ---- signed zeros
    ("(-0.0f32).to_bits()", "u32", 0x80000000, REF_NEG + ": negation of a float literal"),
    ("(0.0f32 + -0.0f32).to_bits()", "u32", 0x00000000, "IEEE-754 6.3: x + (-x) is +0 in round to nearest"),
    ("(-0.0f32 + -0.0f32).to_bits()", "u32", 0x80000000, "IEEE-754 6.3: a sum of like-signed zeros keeps the sign"),
    ("(0.0f32 - 0.0f32).to_bits()", "u32", 0x00000000, "IEEE-754 6.3"),
    ("(-0.0f32 * 5.0f32).to_bits()", "u32", 0x80000000, "IEEE-754 6.3: the sign of a product is the xor of the signs"),
    ("(1.0f32 / -0.0f32).to_bits()", "u32", 0xFF800000, "IEEE-754 7.3: division by zero gives a signed infinity"),
    ("0.0f32 == -0.0f32", "bool", True, "IEEE-754 5.11: zeros compare equal whatever their sign"),
    # ---- round / floor / ceil / trunc
    ("(2.5f32).round().to_bits()", "u32", 0x40400000, "std f32::round: half-way cases away from 0.0 -> 3.0"),
    ("(-1.5f32).round().to_bits()", "u32", 0xC0000000, "std f32::round: half-way cases away from 0.0 -> -2.0"),
    ("(0.5f64).round() as i32", "i32", 1, "std f64::round: half-way cases away from 0.0"),
    ("(-0.4f32).round().to_bits()", "u32", 0x80000000, "std f32::round: -0.4 rounds to -0.0"),
    ("(-1.5f32).floor().to_bits()", "u32", 0xC0000000, "std f32::floor: -2.0"),
    ("(-1.5f32).ceil().to_bits()", "u32", 0xBF800000, "std f32::ceil: -1.0"),
    ("(-1.5f32).trunc().to_bits()", "u32", 0xBF800000, "std f32::trunc: -1.0"),
    ("(1.5f64).floor() as i32", "i32", 1, "std f64::floor"),
    # ---- >> / % on negatives, the euclidean forms
    ("-7i32 >> 1", "i32", -4, REF_ARITH + ": arithmetic right shift on signed integer types"),
    ("-1i32 >> 31", "i32", -1, REF_ARITH + ": arithmetic right shift"),
    ("(-1i32 as u32) >> 31", "u32", 1, REF_ARITH + ": logical right shift on unsigned integer types"),
    ("0xF0u8 >> 4", "u8", 15, REF_ARITH),
    ("-7i32 / 2", "i32", -3, REF_ARITH + ": integer division rounds towards zero"),
    ("-7i32 / -2", "i32", 3, REF_ARITH),
    ("-7i32 % 2", "i32", -1, REF_ARITH + ": the remainder has the sign of the dividend"),
    ("7i32 % -2", "i32", 1, REF_ARITH + ": the remainder has the sign of the dividend"),
    ("(-7i32).rem_euclid(2)", "i32", 1, "std i32::rem_euclid: the least nonnegative remainder"),
    ("7i32.rem_euclid(-2)", "i32", 1, "std i32::rem_euclid"),
    ("(-7i32).div_euclid(2)", "i32", -4, "std i32::div_euclid: -7 = 2 * -4 + 1"),
    # ---- wrapping / checked / saturating
    ("i32::MAX.wrapping_add(1)", "i32", -2147483648, "std i32::wrapping_add"),
    ("200u8.wrapping_add(100)", "u8", 44, "std u8::wrapping_add"),
    ("0u8.wrapping_sub(1)", "u8", 255, "std u8::wrapping_sub"),
    ("0x10000i32.wrapping_mul(0x10000)", "i32", 0, "std i32::wrapping_mul: 2^32 mod 2^32"),
    ("0x10001i32.wrapping_mul(0x10001)", "i32", 0x20001, "std i32::wrapping_mul: 2^32 + 2^17 + 1 mod 2^32"),
    ("i32::MIN.wrapping_abs()", "i32", -2147483648, "std i32::wrapping_abs: MIN stays MIN"),
    ("i32::MIN.wrapping_neg()", "i32", -2147483648, "std i32::wrapping_neg"),
    ("1u32.wrapping_shl(33)", "u32", 2, "std u32::wrapping_shl: the shift amount is taken mod 32"),
    ("0x80000000u32.wrapping_shr(33)", "u32", 0x40000000, "std u32::wrapping_shr: the shift amount is taken mod 32"),
    ("(-8i32).wrapping_shr(1)", "i32", -4, "std i32::wrapping_shr: arithmetic"),
    ("i32::MAX.checked_add(1).is_none()", "bool", True, "std i32::checked_add"),
    ("5u8.checked_sub(6).is_none()", "bool", True, "std u8::checked_sub"),
    ("100u8.checked_mul(2) == Some(200)", "bool", True, "std u8::checked_mul"),
    ("100u8.checked_mul(3).is_none()", "bool", True, "std u8::checked_mul"),
    ("i32::MIN.checked_abs().is_none()", "bool", True, "std i32::checked_abs"),
    ("250u8.saturating_add(10)", "u8", 255, "std u8::saturating_add"),
    ("5u8.saturating_sub(6)", "u8", 0, "std u8::saturating_sub"),
    ("i32::MIN.saturating_sub(1)", "i32", -2147483648, "std i32::saturating_sub"),
    ("i16::MAX.saturating_add(1)", "i16", 32767, "std i16::saturating_add"),
    # ---- bit counting and permutation
    ("1u32.leading_zeros()", "u32", 31, "std u32::leading_zeros"),
    ("0u32.leading_zeros()", "u32", 32, "std u32::leading_zeros"),
    ("0u8.leading_zeros()", "u32", 8, "std u8::leading_zeros: counts within the type's width"),
    ("(-1i32).leading_zeros()", "u32", 0, "std i32::leading_zeros"),
    ("0x1fu8.leading_zeros()", "u32", 3, "std u8::leading_zeros (the FLAC UTF-8 length mask)"),
    ("8u32.trailing_zeros()", "u32", 3, "std u32::trailing_zeros"),
    ("0u16.trailing_zeros()", "u32", 16, "std u16::trailing_zeros"),
    ("0xF0F0u16.count_ones()", "u32", 8, "std u16::count_ones"),
    ("(-1i64).count_ones()", "u32", 64, "std i64::count_ones"),
    ("1u8.reverse_bits()", "u8", 128, "std u8::reverse_bits"),
    ("0x12345678u32.reverse_bits()", "u32", 0x1E6A2C48, "std u32::reverse_bits: 0001 0010 ... 0111 1000 read backwards"),
    ("0x12345678u32.rotate_left(8)", "u32", 0x34567812, "std u32::rotate_left"),
    ("0x81u8.rotate_left(1)", "u8", 0x03, "std u8::rotate_left"),
    ("0x12345678u32.rotate_right(4)", "u32", 0x81234567, "std u32::rotate_right"),
    ("0x12345678u32.swap_bytes()", "u32", 0x78563412, "std u32::swap_bytes"),
    ("0x1234u16.swap_bytes()", "u16", 0x3412, "std u16::swap_bytes"),
    ("u32::from_le_bytes([1, 2, 3, 4])", "u32", 0x04030201, "std u32::from_le_bytes"),
    ("u16::from_be_bytes([0x12, 0x34])", "u16", 0x1234, "std u16::from_be_bytes"),
    ("2i32.pow(10)", "i32", 1024, "std i32::pow"),
    ("(-5i32).abs()", "i32", 5, "std i32::abs"),
    # ---- `!` on typed literals and on literals whose type comes from the context
    ("!0u8", "u8", 255, REF_NEG + ": bitwise NOT on integer types"),
    ("!0i32", "i32", -1, REF_NEG),
    ("!0x0Fu8", "u8", 0xF0, REF_NEG),
    ("!5i8", "i8", -6, REF_NEG),
    ("!true", "bool", False, REF_NEG + ": logical NOT on bool"),
    ("!((1 << 3) - 1)", "u8", 0xF8, REF_NEG + "; the literals take the return type u8 (Rust Reference, 'Integer literal expressions')"),
    ("!((1 << 7) - 1) ^ (1 << 7)", "u8", 0x00, REF_NEG + "; unary ! binds tighter than ^: 0x80 ^ 0x80"),
    ("{ let m: u16 = !0; m }", "u16", 65535, REF_NEG + "; the literal takes the declared type"),
    ("{ let m: u32 = !0xff; m }", "u32", 0xFFFFFF00, REF_NEG),
    ("{ let x: u16 = 0x1234; x & !0xff }", "u16", 0x1200, REF_NEG + "; the literal takes the other operand's type"),
    ("{ let x: u32 = 5; x | !0 }", "u32", 0xFFFFFFFF, REF_NEG),
    ("{ let x: i64 = 0x1_0000_0080; x & !0xffff_ffff }", "i64", 0x100000000, REF_NEG + " (symphonia-core util.rs clamp_i32's test)"),
    # ---- precedence
    ("-1i32 as u32 >> 31", "u32", 1, REF_PREC + ": unary - over `as` over >>"),
    ("-5i32 as u8", "u8", 251, REF_PREC + ": unary - over `as`"),
    ("-5i32.pow(2)", "i32", -25, REF_PREC + ": method calls over unary -"),
    ("-2i32.abs()", "i32", -2, REF_PREC + ": method calls over unary -"),
    ("1u32 << 2 + 1", "u32", 8, REF_PREC + ": + over <<"),
    ("2i32 + 3 << 1", "i32", 10, REF_PREC + ": + over <<"),
    ("1u8 as u32 + 255", "u32", 256, REF_PREC + ": `as` over +"),
    ("3u8 as u32 * 100", "u32", 300, REF_PREC + ": `as` over *"),
    ("6i32 & 3 == 2", "bool", True, REF_PREC + ": & over == (unlike C)"),
    ("1i32 | 2 ^ 3 & 4", "i32", 3, REF_PREC + ": & over ^ over |"),
    ("1u32 << 4 >> 2", "u32", 4, REF_PREC + ": shifts associate left to right"),
    ("100i32 - 10 - 1", "i32", 89, REF_PREC + ": - associates left to right"),
    # ---- NaN in min / max / clamp / comparisons, signum
    ("f32::NAN.max(1.0f32).to_bits()", "u32", 0x3F800000, "std f32::max: if one of the arguments is NaN, the other is returned"),
    ("1.0f32.min(f32::NAN).to_bits()", "u32", 0x3F800000, "std f32::min: if one of the arguments is NaN, the other is returned"),
    ("f32::NAN.min(f32::NAN).is_nan()", "bool", True, "std f32::min"),
    ("f32::NAN == f32::NAN", "bool", False, "IEEE-754 5.11: NaN is unordered"),
    ("f32::NAN != f32::NAN", "bool", True, "IEEE-754 5.11"),
    ("f32::NAN < 1.0f32", "bool", False, "IEEE-754 5.11"),
    ("5i32.clamp(0, 3)", "i32", 3, "std Ord::clamp"),
    ("(-5i32).clamp(0, 3)", "i32", 0, "std Ord::clamp"),
    ("2.5f32.clamp(0.0, 1.0).to_bits()", "u32", 0x3F800000, "std f32::clamp"),
    ("(-0.5f64).clamp(-1.0, 1.0).to_bits()", "u64", 0xBFE0000000000000, "std f64::clamp"),
    ("f32::NAN.clamp(0.0, 1.0).is_nan()", "bool", True, "std f32::clamp: NaN stays NaN"),
    ("3i32.min(-3)", "i32", -3, "std Ord::min"),
    ("3u8.max(200)", "u8", 200, "std Ord::max"),
    ("(-3i32).signum()", "i32", -1, "std i32::signum"),
    ("0i32.signum()", "i32", 0, "std i32::signum"),
    ("(-0.0f32).signum().to_bits()", "u32", 0xBF800000, "std f32::signum: -1.0 if the number is negative, -0.0 included"),
    ("0.0f32.signum().to_bits()", "u32", 0x3F800000, "std f32::signum: 1.0 if the number is positive, +0.0 included"),
    ("f32::NAN.signum().is_nan()", "bool", True, "std f32::signum"),
    # ---- string literals
    ('"ab \\\n      cd".len()', "usize", 5, REF_LIT + ": a backslash before a line break drops the break and the white space after it"),
    ('b"ab \\\n\t  cd".len()', "usize", 5, REF_LIT + ": the same in a byte string, tabs included"),
    ('"ab \\\n\n   cd".len()', "usize", 5, REF_LIT + ": further line breaks are white space too"),
    ('"abc".len()', "usize", 3, "std str::len: the length in bytes (the quotes are not part of it)"),
    ('"a\\tb\\\\".len()', "usize", 4, REF_LIT + ": \\t and \\\\ are one character each"),
    ('"\\x41\\n".len()', "usize", 2, REF_LIT + ": \\xHH"),
    ('"\\u{e9}".len()', "usize", 2, "std str::len: U+00E9 is two bytes of UTF-8"),
    ('"\\u{1F600}".len()', "usize", 4, "std str::len: U+1F600 is four bytes of UTF-8"),
    ('r"a\\nb".len()', "usize", 4, REF_LIT + ": a raw string has no escapes"),
    ('r#"a"b"#.len()', "usize", 3, REF_LIT + ": raw string delimiters"),
    ('b"\\xff\\0"[0]', "u8", 255, REF_LIT + ": a byte escape"),
    ('b"a\\"b".len()', "usize", 3, REF_LIT + ": a quote escape"),
]


@pytest.mark.parametrize("expr,ty,want,source", PROBES, ids=["%03d: %s" % (i, p[0].replace("\n", "<nl>").replace("\t", "<tab>")) for i, p in enumerate(PROBES)])
def test_rust_arithmetic_probe(expr, ty, want, source):
    it = Interp()
    it.load_source("pub fn probe() -> %s {\n%s\n}\n" % (ty, expr), "probe.rs")
    got = it.call("probe")
    got = bool(got) if ty == "bool" else int(got.v)
    print("%s -> %r, rustc: %r  [%s]" % (expr, got, want, source))
    assert got == want and type(got) is type(want)
    assert it.overflows == 0


def test_the_probe_table_is_as_large_as_it_claims():
    assert len(PROBES) >= 80 and len({p[0] for p in PROBES}) == len(PROBES)
    assert all(p[3] for p in PROBES), "every expectation names where it comes from"


# ---------------------------------------------------------------- the interpreter's own panics
PANICS = [
    ("assert!(false);", "assert!"),
    ("assert!(1 + 1 == 3, \"with a message\");", "assert! with a message"),
    ("assert_eq!(1, 2);", "assert_eq!"),
    ("assert_ne!(2, 2);", "assert_ne!"),
    ("debug_assert!(false);", "debug_assert! (tests build with debug assertions on)"),
    ("debug_assert_eq!(1u8, 2u8);", "debug_assert_eq!"),
    ("let r: Result<u32, u32> = Err(1); r.unwrap();", "Result::unwrap on Err"),
    ("let r: Result<u32, u32> = Err(1); r.expect(\"why\");", "Result::expect on Err"),
    ("let o: Option<u32> = None; o.unwrap();", "Option::unwrap on None"),
    ("let v = [1u8, 2, 3]; let i = 3; let _x = v[i];", "index past the end of an array"),
    ("let v = vec![1u8, 2, 3]; let s = &v[..]; let _x = s[7];", "index past the end of a slice"),
    ("let v = [1u8, 2, 3]; let _s = &v[1..5];", "slice range past the end"),
    ("let v = [1u8, 2, 3]; let (a, b) = (2, 1); let _s = &v[a..b];", "slice range that starts after its end"),
    ("let d = 0i32; let _x = 1i32 / d;", "integer division by zero"),
    ("let d = 0u32; let _x = 1u32 % d;", "integer remainder by zero"),
    ("panic!(\"boom\");", "panic!"),
    ("unreachable!();", "unreachable!"),
    ("let mut d = [0u8; 2]; d.copy_from_slice(&[1u8, 2, 3]);", "copy_from_slice of another length"),
]


@pytest.mark.parametrize("body,what", PANICS, ids=[p[1] for p in PANICS])
def test_the_interpreter_panics_where_rust_does(body, what):
    it = Interp()
    it.load_source("pub fn probe() {\n%s\n}\n" % body, "probe.rs")
    with pytest.raises(RustPanic):
        it.call("probe")


def test_a_passing_assertion_does_not_panic():
    """the other side of the panics above: the same shapes with true conditions return normally"""
    it = Interp()
    it.load_source("pub fn probe() -> u32 { assert!(true); assert_eq!(2, 1 + 1); debug_assert!(1 < 2); let v = [1u8, 2, 3]; "
                   "let r: Result<u32, u32> = Ok(5); let _s = &v[1..3]; r.unwrap() + u32::from(v[2]) }", "probe.rs")
    assert it.call("probe").v == 8


OVERFLOWS = [
    ("let a = i32::MAX; let b = 1i32; let _c = a + b;", "i32 sum"),
    ("let a = 200u8; let b = 100u8; let _c = a + b;", "u8 sum"),
    ("let a = 0u32; let b = 1u32; let _c = a - b;", "u32 difference below zero"),
    ("let a = 0x10000i32; let _c = a * a;", "i32 product"),
    ("let a = i32::MIN; let _c = -a;", "negation of i32::MIN"),
    ("let a = 1u32; let s = 32u32; let _c = a << s;", "shift by the type's width"),
]


@pytest.mark.parametrize("body,what", OVERFLOWS, ids=[p[1] for p in OVERFLOWS])
def test_an_implicit_integer_overflow_is_counted(body, what):
    """A debug build panics on these ('attempt to add with overflow').  The interpreter does NOT raise: it wraps, as a release build
    does, and counts the event in Interp.overflows -- the fixture generator and the reference-unit-test cases assert that count is 0."""
    it = Interp()
    it.load_source("pub fn probe() {\n%s\n}\n" % body, "probe.rs")
    it.call("probe")
    assert it.overflows == 1


def test_explicitly_wrapping_arithmetic_is_not_counted():
    it = Interp()
    it.load_source("pub fn probe() -> i32 { let a = i32::MAX; let w = std::num::Wrapping(a) + std::num::Wrapping(1i32); "
                   "a.wrapping_add(1).wrapping_mul(3) ^ w.0 ^ (300i32 as u8 as i32) }", "probe.rs")
    it.call("probe")
    assert it.overflows == 0
