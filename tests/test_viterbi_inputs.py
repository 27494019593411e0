"""The inputs of tests/test_gpu_viterbi_rows.py, checked without a GPU: by a NumPy max-plus reference whose tie rule can be switched
(tests/viterbi_cases.py), the fixtures can catch the faults they are meant for.  On the grid of weights exact ties are frequent in
rows of every lane-group width, and in different lanes of a row; a wrong tie rule, a reduction that forgets lanes, a lost last pdf
and a wrong seam of the back-trace ring each change a best path that the GPU tests compare.  These are conditions on the fixtures,
not measurements of the kernels: if one fails, the fixture is too weak."""
import numpy as np
import pytest

import graphs
import viterbi_cases as vc

_refs = {}


def refs1(wl, name, quant=True, rule="lowest"):
    """The reference's results for the utterances of group 1 of `name`, once."""
    key = (name, quant, rule)
    if key not in _refs:
        g, V, lens = vc.case1(wl, name, quant)
        _refs[key] = [vc.reference(g, V[b], int(L), rule) for b, L in enumerate(lens)]
    return _refs[key]


def counts_by_lg(g, results, on_path=False):
    """{lg: (tied live cells, those with the two lowest maximisers in different lanes)} over the utterances' (frame, row) cells;
    on_path: only the cells of the best paths (the back-pointers the chase follows)."""
    t = vc.tables(g)
    out = {}
    for lg in sorted(set(t.lg[t.deg > 0].tolist())):
        rows = t.lg == lg
        tied = cross = 0
        for r in results:
            if on_path:
                L = r.path.size
                if L == 0 or r.path[0] < 0:
                    continue
                n = np.arange(1, L + 1)
                s = np.concatenate([r.path[1:], [t.S]])  # the state whose back-pointer at row n names path[n - 1]
                m = rows[s]
                tied += int(r.tied[n, s][m].sum())
                cross += int(r.cross[n, s][m].sum())
            else:
                tied += int(r.tied[:, rows].sum())
                cross += int(r.cross[:, rows].sum())
        out[lg] = (tied, cross)
    return out


def test_the_reference_is_the_oracle_under_the_specified_rule(wl, oracle):
    o, oc = oracle
    for name in ("small15", "den24", "widths"):
        g, V, lens = vc.case1(wl, name)
        of = graphs.to_oracle(o, g, "tropical", np.float32)
        for b, L in enumerate(lens):
            pr, sr, bpr = oc.viterbi(of, g.state2pdf, g.P, V[b], int(L), dtype=np.float32)
            r = refs1(wl, name)[b]
            assert np.array_equal(r.path, pr[:L]) and (pr[L:] == -1).all() and r.score == sr
            assert np.array_equal(r.bp[1:], bpr[1 : L + 1])


@pytest.mark.parametrize("name", vc.GROUP1)
def test_ties_in_every_group_width(wl, name):
    """C.1: for every lane-group width of the fixture at least 20 tied live cells, at least 5 of them across lanes (lg >= 1: a row
    on one lane has no other lane)."""
    g = vc.graph(wl, name)
    t = vc.tables(g)
    assert int(t.deg.max()) <= 255
    c = counts_by_lg(g, refs1(wl, name))
    live = sum(int(r.live.sum()) for r in refs1(wl, name))
    print(f"{name}: {live} live cells; lg: (tied, tied across lanes) {c}; on the best paths {counts_by_lg(g, refs1(wl, name), True)}")
    for lg, (tied, cross) in c.items():
        assert tied >= 20, (name, lg, tied)
        assert lg == 0 or cross >= 5, (name, lg, cross)


def test_group_widths_of_the_fixtures(wl):
    """lg 1 .. 6 all occur, lg 5 in the small denominator graphs and in `widths`, and on the best paths every one of them has a
    tie across lanes in some fixture: the second butterfly of the reduction decides a back-pointer that the chase follows."""
    have = {name: set(vc.tables(vc.graph(wl, name)).lg.tolist()) for name in vc.GROUP1}
    assert have["den24"] >= {0, 1, 2, 3, 4, 5} and have["den60"] == set(range(7)) and have["widths"] == set(range(7)), have
    assert 4 in have["lex15"]
    on_path = {}
    for name in vc.GROUP1:
        for lg, (tied, cross) in counts_by_lg(vc.graph(wl, name), refs1(wl, name), True).items():
            on_path[lg] = on_path.get(lg, 0) + cross
    print("ties across lanes on the best paths, by lg:", on_path)
    assert all(on_path[lg] >= 1 for lg in range(1, 7)), on_path


def test_every_width_of_widths_has_ties(wl):
    """C.2: the rows of 4 .. 255 arcs of `widths` each have tied cells, across lanes where the row has lanes."""
    g = vc.graph(wl, "widths")
    t = vc.tables(g)
    for i, width in enumerate(vc.WIDTHS):
        s = 10 + 3 * i
        assert t.deg[s] == width and t.lg[s] == vc.lg_of(width)
        tied = sum(int(r.tied[:, s].sum()) for r in refs1(wl, "widths"))
        cross = sum(int(r.cross[:, s].sum()) for r in refs1(wl, "widths"))
        print(f"widths: row of {width} arcs (lg {t.lg[s]}): {tied} tied cells, {cross} across lanes")
        assert tied >= 1 and (width <= 4 or cross >= 1), (width, tied, cross)
    assert [vc.lg_of(w) for w in vc.WIDTHS] == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    assert int(vc.tables(vc.graph(wl, "widths256")).deg.max()) == 256


def _changed(wl, name, rule):
    base, mut = refs1(wl, name), refs1(wl, name, True, rule)
    assert all(a.score == b.score for a, b in zip(base, mut))  # (the rule names another arc of the same value)
    return [not np.array_equal(a.path, b.path) for a, b in zip(base, mut)]


@pytest.mark.parametrize("name", vc.GROUP1)
def test_a_wrong_tie_rule_changes_the_paths(wl, name):
    """C.3 and C.4: "highest source among ties" changes the best path of at least half of the utterances; a reduction that keeps
    only the lane of arc 0 changes at least one."""
    high, lane0 = _changed(wl, name, "highest"), _changed(wl, name, "lane0")
    print(f"{name}: paths changed under 'highest source': {sum(high)} of {len(high)}, under 'lane of arc 0 only': {sum(lane0)}")
    assert 2 * sum(high) >= len(high), high
    assert sum(lane0) >= 1, lane0


@pytest.mark.parametrize("name", vc.GROUP1)
def test_the_continuous_weights_have_no_ties(wl, name):
    """C.5: with the weights the builders ship, ties are float32 coincidences -- fewer than one live cell in 10 000, against 4 to
    40 in 100 on the grid -- and none lies on a best path: the earlier Viterbi tests, whose emissions alone were on a grid, never
    asked the tie rule anything that a path or a score could show."""
    results = refs1(wl, name, False)
    tied = sum(int(r.tied.sum()) for r in results)
    live = sum(int(r.live.sum()) for r in results)
    on_path = sum(t for t, _ in counts_by_lg(vc.graph(wl, name, False), results, True).values())
    print(f"{name}, continuous weights: {tied} tied cells of {live} live ones, {on_path} on the best paths")
    assert tied * 10000 < live and on_path == 0


@pytest.mark.parametrize("name,P", vc.P_CASES)
def test_the_last_pdf_and_every_block_of_64_are_on_the_paths(wl, name, P):
    """C.7: the best paths pass a state of pdf P - 1 and of every block of 64 pdfs, and without pdf P - 1 a path or a score changes."""
    g, V, lens = vc.case_pdfs(wl, name, P)
    base = [vc.reference(g, V[b], int(L)) for b, L in enumerate(lens)]
    pdfs = np.unique(np.concatenate([np.asarray(g.state2pdf)[r.path[r.path >= 0]] for r in base]))
    print(f"{name}, P = {P}: the best paths visit {pdfs.size} pdfs, blocks {sorted(set((pdfs // 64).tolist()))}")
    assert P - 1 in pdfs and set((pdfs // 64).tolist()) == set(range((P + 63) // 64))
    Vm = V.copy()
    Vm[..., P - 1] = -np.inf
    mut = [vc.reference(g, Vm[b], int(L)) for b, L in enumerate(lens)]
    assert any(a.score != b.score or not np.array_equal(a.path, b.path) for a, b in zip(base, mut))


@pytest.mark.parametrize("name", sorted(vc.RING_R))
def test_a_wrong_seam_of_the_ring_changes_the_path(wl, name):
    """C.8: the chunks of the back-trace (R frames each, the first one partial) have their seams at the frames hi - R.  With the
    row of a seam cut out -- the chase reads its neighbour's -- the path of every utterance that has a seam changes."""
    g, V, lens = vc.case_ring(wl, name)
    R = vc.RING_R[name]
    chunks = []
    for b, L in enumerate(lens):
        L = int(L)
        seams = vc.seam_frames(L, R)
        chunks.append(len(seams) + 1)
        base = vc.reference(g, V[b], L)
        assert base.score > -np.inf, (name, b)
        if not seams:
            continue
        for f in seams:  # each seam alone
            assert not np.array_equal(vc.reference(g, V[b], L, seams=(f,)).path, base.path), (name, b, L, f)
    print(f"{name}: R = {R}, lens {lens.tolist()}, chunks {chunks}")
    want = {1, 2, 3} if name == "den60" else {1, 2, 3, 5}
    assert set(chunks) >= want, chunks
    # a first chunk (the last one chased) of one frame: the kernel's frame 2 alone
    assert any(vc.seam_frames(int(L), R)[-1:] == [1] for L in lens)
