"""polish.ChainOptions and polish.PASSES: the one list of the chain's opt-in stages and the one table of its count-carrying
passes, checked against everything that is derived from them. No device is touched."""
import dataclasses
import itertools

import numpy as np
import pytest

from pepper_thesis_amd import polish, polish_edits as pe, runtime

# every option at a set value
SET = dict(qualities=True, edits=True, evidence=True, min_depth=3, min_qual=20, min_support=2, use_hp=True, vote=True, vote_runs=3)


def _refused(kw: dict) -> bool:
    """the three sets no chain is made for"""
    return bool(("vote_runs" in kw and "vote" not in kw) or ("vote_runs" in kw and "min_support" in kw)
                or ("evidence" in kw and "edits" not in kw))


def test_every_option_set_gives_its_keywords_or_is_refused():
    assert tuple(f.name for f in dataclasses.fields(polish.ChainOptions)) == tuple(SET)
    n_refused = 0
    for on in itertools.product((False, True), repeat=len(SET)):
        kw = {k: v for (k, v), use in zip(SET.items(), on) if use}
        if _refused(kw):
            n_refused += 1
            with pytest.raises(ValueError):
                polish.ChainOptions(**kw)
            continue
        o = polish.ChainOptions(**kw)
        assert o.keywords() == kw
        assert o.want_counts == any(k in kw for k in ("evidence", "min_support", "vote"))
        assert o.want_depth == (o.want_counts or "min_depth" in kw)
        assert o.want_row_qual == ("qualities" in kw or "min_qual" in kw)
    # each refusal fixes two of the nine options (128 sets), two of them four (64 or 32), all three five (16)
    assert n_refused == 3 * 128 - (64 + 32 + 32) + 16


def test_the_refusals_keep_their_texts():
    for kw, text in ((dict(vote_runs=3), "a chain with vote_runs needs vote"),
                     (dict(vote=True, vote_runs=3, min_support=2), "a chain with vote_runs takes no min_support"),
                     (dict(evidence=True), "a chain with evidence needs edits")):
        with pytest.raises(ValueError, match=text):
            polish.ChainOptions(**kw)


def test_options_of_a_namespace():
    from pepper_thesis_amd import cli
    base = ["-b", "r.bam", "-f", "r.fa", "-o", "out"]
    args = cli.polish_parser().parse_args(base + ["-m", "m.npz"])
    assert polish.ChainOptions.from_args(args).keywords() == {}
    args = cli.polish_parser().parse_args(base + ["--vote", "--runs", "--edits", "--evidence", "--qualities", "--min_depth", "3", "-hp"])
    assert polish.ChainOptions.from_args(args).keywords() == dict(qualities=True, edits=True, evidence=True, min_depth=3, use_hp=True,
                                                                 vote=True, vote_runs=3)
    args = cli.polish_parser().parse_args(base + ["--vote", "--runs", "--min_run", "5", "--min_qual", "20", "--min_support", "2"])
    o = polish.ChainOptions.from_args(args)   # not refused here: the command says so in its own words
    assert o.keywords() == dict(min_qual=20, min_support=2, vote=True, vote_runs=5)
    with pytest.raises(ValueError):
        polish.ChainOptions(**o.keywords())


def _full_result():
    """a result that carries every extra plane, each with values of its own"""
    res = polish.ChainResult(np.array([0, 2]), b"AC", b"\x05\x06", np.array([0, 1]), np.zeros(1, pe.EDIT_DTYPE))
    values = {"evidence": np.array([(9, 1, 5, 1)], pe.EVIDENCE_DTYPE)}
    for i, p in enumerate(polish.PASSES):
        values[p.attr] = tuple(10 * (i + 1) + j for j in range(len(p.timers)))
    for name, v in values.items():
        res = getattr(polish, "with_" + name)(res, v)
    return res, values


def test_every_pass_row_is_consistent():
    assert polish.ChainResult._fields == ("region_off", "bases", "qual", "edit_off", "edits")
    assert polish.RESULT_EXTRAS == tuple(p.attr for p in polish.PASSES) + ("evidence",)
    plain = polish.ChainResult(np.array([0, 2]), b"AC")
    full, values = _full_result()
    assert tuple(full)[:3] == (full.region_off, b"AC", b"\x05\x06") and len(full.region(0)) == 4
    keys = [k for p in polish.PASSES for k in p.timers]
    assert len(set(keys)) == len(keys) == len(polish.PASS_TIMERS)
    for p in polish.PASSES:
        assert p.option in SET and getattr(plain, p.attr) is None
        assert len(p.pick) == len(p.timers) == len(p.empty) and max(p.pick) < p.n_counters and not {1, 2} & set(p.pick)
        assert p.in_place is None or callable(getattr(runtime.Context, p.in_place))
        T = polish._timers(None)
        assert all(T[k] == 0 for k in p.timers)
        # a result that carries the row's counts, counted twice, and one that does not
        counts = tuple(range(3, 3 + len(p.timers)))
        got = getattr(polish, "with_" + p.attr)(plain, counts)
        assert getattr(got, p.attr) == counts and tuple(got) == tuple(plain)
        for r in (got, plain, got):
            polish._count_masked(T, r)
        assert [T[k] for k in p.timers] == [2 * c for c in counts]
        assert all(T[k] == 0 for k in polish.PASS_TIMERS if k not in p.timers)
        # the log line is filled from the option and the row's timers
        assert p.report % dict(SET, draft_regions=0, **T)
    # setting one plane keeps every other plane of a result that carries them all
    for name in polish.RESULT_EXTRAS:
        new = values["evidence"].copy() if name == "evidence" else tuple(v + 100 for v in values[name])
        got = getattr(polish, "with_" + name)(full, new)
        assert tuple(got) == tuple(full)
        for other in polish.RESULT_EXTRAS:
            want = new if other == name else values[other]
            assert getattr(got, other) is want or getattr(got, other) == want, (name, other)


def _no_chunk_chain(**kw):
    chain = object.__new__(polish._DeviceChain)   # (no context: the path launches nothing)
    chain.options = polish.ChainOptions(**kw)
    return chain


@pytest.mark.parametrize("kw", [
    {},
    dict(qualities=True, edits=True, evidence=True, min_depth=3, min_qual=20, min_support=2),
    dict(vote=True, vote_runs=3, qualities=True, edits=True, evidence=True, min_depth=3, min_qual=2),
], ids=["none", "model", "vote"])
def test_a_launch_without_chunks_gives_every_plane_empty(kw):
    res = _no_chunk_chain(**kw)._labels_and_stitch(None, 0, 3)
    assert res.region_off.dtype == np.int64 and res.region_off.tolist() == [0, 0, 0, 0] and res.bases == b""
    assert res.qual == (b"" if "qualities" in kw else None)
    if "edits" in kw:
        assert res.edit_off.dtype == np.int64 and res.edit_off.tolist() == [0, 0, 0, 0] and res.edit_off is not res.region_off
        assert res.edits.dtype == pe.EDIT_DTYPE and len(res.edits) == 0
        assert res.evidence.dtype == pe.EVIDENCE_DTYPE and len(res.evidence) == 0
    else:
        assert res.edit_off is None and res.edits is None and res.evidence is None
    for p in polish.PASSES:
        assert getattr(res, p.attr) == ((0,) * len(p.timers) if p.option in kw else None), p.attr
    assert res.region(1)[0] == b""
