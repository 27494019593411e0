"""The pdf-major table of the pair forms (mm_rows.cpp make_rows / set_partner, RowGraph::pdftab): what the pair kernels' phase B
sums the posteriors through since it keeps no q vector.  For the forward and the backward form: the table is a permutation of the
rows, the rows inside a pdf's range of `pdfse` have that pdf, the ranges tile the table, and an entry's own and partner halves
are the position fields of slot words 0 and 1 of the same row."""
import numpy as np
import pytest

GRAPHS = {
    "lfmmi_600_40_s5": lambda wl: wl.lfmmi_denominator(600, 40, seed=5),
    "lfmmi_600_200_s5": lambda wl: wl.lfmmi_denominator(600, 200, seed=5),
    "lfmmi_600_10_s5": lambda wl: wl.lfmmi_denominator(600, 10, seed=5),
}


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_pdf_major_table(mm, wl, gname, d):
    g = GRAPHS[gname](wl)
    f = wl.to_fsm(mm, g)
    cf = mm.compile(f, mm.statemap(g.state2pdf, g.P))
    tab, pdfse, slots = cf.pair_pdf_table(d)
    S1, P1 = f.S1, g.P + 1
    own, partner = tab & 0xFFFF, tab >> 16
    assert (own % 8 == 0).all() and (partner % 8 == 0).all()
    # a permutation of the rows, in both numberings
    assert np.array_equal(np.sort(own // 8), np.arange(S1)) and np.array_equal(np.sort(partner // 8), np.arange(S1))
    # slot words of the finishing lanes: word 0 = 8 * position | (8 * pdf) << 16, word 1 = 8 * partner position | (8 * place in the table) << 16
    assert slots.shape == (S1, 2)
    pos8, pdf = slots[:, 0] & 0xFFFF, (slots[:, 0] >> 16) // 8
    place = (slots[:, 1] >> 16) // 8
    assert np.array_equal(np.sort(place), np.arange(S1))
    assert np.array_equal(own[place], pos8) and np.array_equal(partner[place], slots[:, 1] & 0xFFFF)
    # the ranges of pdfse: every row of a range has the range's pdf, and the ranges tile the table
    pdf_of_place = np.empty(S1, dtype=np.int64)
    pdf_of_place[place] = pdf
    assert pdfse.shape == (P1, 2)
    covered = np.zeros(S1, dtype=np.int64)
    for p in range(P1):
        a, b = int(pdfse[p, 0]), int(pdfse[p, 1])
        assert 0 <= a <= b <= S1
        assert (pdf_of_place[a:b] == p).all()
        covered[a:b] += 1
        assert b - a == int((pdf_of_place == p).sum())
    assert (covered == 1).all()
