"""CPU: every case of assess_limits_cases, run through the restatements alone, shows what it was built for (the default geometry,
a window of 65 trips with two hits in one lane, more than 256 pairs, more anchors than the chain stages, the segment range's
ends), so a case that stops reaching its kernel path fails here; and the byte-equal shortcut gives what the rule gives."""
import numpy as np
import pytest

import assess_errors_ref as E
import assess_limits_cases as Z
import assess_ref as R


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_every_case_shows_what_it_was_built_for(name):
    x = Z.expected(name)   # (runs the case's own check)
    assert x.errors == (name in Z.WITH_ERRORS)
    assert len(x.off) == len(x.pairs) + 1 and x.off[-1] == len(x.rows) <= Z.slots_of(x.pairs, x.L)
    assert np.array_equal(x.rows[:, 13], np.repeat(np.arange(len(x.pairs)), np.diff(x.off)))
    if x.errors:
        # the two restatements walk their own tracebacks: the records they count are the same
        per_pair = np.array([np.bincount(x.err_rows[x.err_off[p]:x.err_off[p + 1], 4], minlength=4)[1:] for p in range(len(x.pairs))])
        assert np.array_equal(per_pair.reshape(-1, 3), x.tot[:, 5:8])
        assert np.array_equal(x.hist[:, :, 0].sum(axis=1), x.tot[:, 4] + x.tot[:, 5] + x.tot[:, 6])
        assert np.array_equal(x.hist[:, :, 1:].sum(axis=1), x.tot[:, 5:8])
        for p in np.nonzero(x.tot[:, 2] == 0)[0][:40]:   # the patch property, on the first pairs that are aligned throughout
            recs = [dict(zip(E.ERR_FIELDS, (int(v) for v in r))) for r in x.err_rows[x.err_off[p]:x.err_off[p + 1]]]
            assert E.apply_errors(x.pairs[p][0], recs) == x.pairs[p][1], (name, p)


def test_segment_heights_cross_the_flush_and_the_reload():
    """k_as_sweep stores a direction word every eight rows and at the last, and reloads its bytes every 64 rows"""
    x = Z.expected("grid")
    aligned = x.rows[x.rows[:, 4] == R.SEG_ALIGNED]
    heights = set(int(v) for v in aligned[:, 2])
    assert heights == set(Z.GRID_N)
    assert {h % 8 for h in heights} >= {0, 1, 7} and {7, 8, 9, 63, 64, 65, 127, 128, 129} <= heights
    for h in (0, 1, 8, 64, 65, 128, 130):   # every height meets both ends of the aligned range of d
        ds = set(int(v) for v in (aligned[aligned[:, 2] == h][:, 3] - h))
        assert ds == {d for d in Z.GRID_D if h + d >= 0 and d != 97}, (h, sorted(ds))


def test_a_prefix_of_the_grid_is_the_rule_on_the_prefix():
    x = Z.expected("grid")
    y = Z.prefix(x, 257)
    rows, off, tot = R.assess_batch(x.pairs[:257], x.L, x.shift)
    assert np.array_equal(y.rows, rows) and np.array_equal(y.off, off) and np.array_equal(y.tot, tot)
    assert [len(Z.prefix(x, k).pairs) for k in Z.GRID_PREFIXES] == [255, 256, 257, 1025]


def test_the_byte_equal_shortcut_is_the_rule():
    x = Z.expected("staged")
    A, B = x.pairs[1]
    Q = x.quals[1]
    segs = R.segments(len(A), len(B), R.chain(R.find_anchors(A, B, x.L, x.shift)))
    equal = [s for s in segs if Z.byte_equal(A, B, *s[:4])]
    assert len(equal) > 900 and len(equal) < len(segs)
    picked = equal[:3] + equal[500:503] + equal[-2:] + [(1000, 1000, 0, 0, 32), (len(A), len(B), 0, 0, 0)]
    assert len(picked) >= 8 and any(s[2] == 0 for s in picked)
    for a0, b0, n, m, _ in picked:
        assert Z.align_or_equal(A, B, a0, b0, n, m) == R.align_segment(A, B, a0, b0, n, m), (a0, n)
        assert Z.walk_or_equal(A, B, a0, b0, n, m, Q, 1, 7) == E.walk_segment(A, B, a0, b0, n, m, Q, 1, 7), (a0, n)
    # a segment with one difference does not take the shortcut
    other = next(s for s in segs if not Z.byte_equal(A, B, *s[:4]))
    assert Z.align_or_equal(A, B, *other[:4])["match"] < max(other[2], 1)
    # the whole first small pair both ways
    for p in (0, 2):
        assert np.array_equal(R.assess_batch(x.pairs[p:p + 1], x.L, x.shift)[0][:, :13], x.rows[x.off[p]:x.off[p + 1], :13])
