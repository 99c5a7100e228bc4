"""The six scheme parsers split their string into words the way the reference's Istream does: any run of space, \\t, \\n, \\r, \\f, \\v separates
two words, and such a run before the first word or after the last is ignored.  Host only, no GPU.  The messages of what they refuse are
asserted by each scheme's own test."""
import ctypes as C

import pytest

WHITESPACE = " \t\n\r\f\v"


def fields(v):
    """a parser's result as plain comparable data (a ctypes structure: its fields, nested ones too)"""
    if isinstance(v, C.Structure):
        return tuple((name, fields(getattr(v, name))) for name, _ in v._fields_)
    return v


def padded(clean):
    """the clean string with every whitespace character leading, trailing and doubled between the words, one character at a time and all
    six together"""
    words = clean.split(" ")
    out = [c + (c + c).join(words) + c for c in WHITESPACE]
    out.append(WHITESPACE + (WHITESPACE + WHITESPACE[::-1]).join(words) + WHITESPACE[::-1])
    return out


@pytest.mark.parametrize("parser,clean", [
    ("sngrad_parse", "limited corrected 0.33"), ("ddt_cn_parse", "CrankNicolson 0.9"), ("ddt_local_parse", "CoEuler phi rho 0.5"),
    ("limiter", "limitedLimitedLinear 0.5 -1 2"), ("grad_limiter", "cellMDLimited Gauss linear 0.5"), ("grad_scheme", "faceLimited leastSquares 0.5")])
def test_whitespace_around_and_between_the_words_changes_nothing(pkg, parser, clean):
    parse = getattr(pkg.engine, parser)
    want = fields(parse(clean))
    for text in padded(clean):
        assert fields(parse(text)) == want, (parser, text)
    with pytest.raises(pkg.engine.MiError):                          # nothing but whitespace is an empty scheme
        parse(WHITESPACE)
