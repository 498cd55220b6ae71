"""The premises of tests/test_domain_edge_gpu.py, on the Python references alone (no GPU): the
solved rows yield their claimed err and delta through every learning reference, the helper inputs
exceed 32 bits where they claim to, the InDomain guard fires on what it is there for, and every
learning case of the GPU file stays in domain on the reference.

The learning cases are built by the same functions from the same seeds as in the GPU file, at the
same n; their tables are numpy arrays (domain_edge.wide_table, flat_table, the solved tables), so
what is proved here is what the GPU file uploads.  Only the "full" / "edge_unset" tables of the
values, act and search tests come from an on-device generator; they feed no learning step."""
import numpy as np
import pytest

import domain_edge as DE
import ntsearch_ref as SRCH
import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR

CASES = DE.learning_cases()


# ------------------------------------------------------------------ solved rows
@pytest.mark.parametrize("lib", DE.LIBS)
@pytest.mark.parametrize("spec", ["2x4", "8x4"])
def test_solved_rows_yield_their_err_and_delta(lib, spec):
    bounds = DE.STAGE_BOUNDS[0] if lib in DE.STAGED_LIBS else None
    case = DE.exact_case(lib, spec, bounds, seed=3)
    ref = DE.RefSide(case, lib)
    first = None
    for c, (call, rows) in enumerate(zip(case.calls, case.rows)):
        before = {} if ref.tc is None else dict(ref.tc.A)
        acts, errs, deltas, state = ref.step(call)  # inside InDomain
        at = [1, 2, 3, 5, 6, 7]                     # rows 0 and 4 have no previous afterstate
        assert [errs[i] for i in at] == [r.err for r in rows]
        assert [deltas[i] for i in at] == [r.delta for r in rows] == list(DE.DELTAS)
        assert errs[0] == errs[4] == 0 and deltas[0] == deltas[4] == 0
        assert all(r.err != 0 for r in rows) and acts[1] == 0
        want = ref.want_lut()
        for r in rows:
            s = () if bounds is None else (ref.net.stage(r.prev),)
            if lib in DE.TC_LIBS and r.delta:
                grown = {ref.tc.A[(*s, *k)] - before.get((*s, *k), 0) for k in r.entries}
                assert grown == {abs(r.delta)}      # 2^31 on the INT32_MIN row
            for k, v in r.entries.items():          # fresh ea: every step is the whole delta
                assert int(want[(*s, *k)]) == v + r.delta
        first = first or rows
    assert first[0].delta == -(1 << 31) and first[0].err == -(1 << 33)
    assert {v for v in first[0].entries.values()} == {(1 << 33) // (8 * len(case.tuples))}


def test_the_issue_s_two_worked_rows():
    """Tuple (0, 1, 2, 3), prev = 1..16: eight entries of 2^30 at lr = 1 / 4 give err = -2^33 and
    delta = INT32_MIN, every entry ending at -2^30; seven of -2^28 and one of -(2^28 - 1) at lr = 1
    give delta = INT32_MAX."""
    tuples, prev = ((0, 1, 2, 3),), list(range(1, 17))
    for entries, lr, err, delta in (([1 << 30] * 8, (1, 2), -(1 << 33), DE.INT32_MIN),
                                    ([-(1 << 28)] * 7 + [1 - (1 << 28)], (1, 0), DE.INT32_MAX,
                                     DE.INT32_MAX)):
        net = NR.Net(tuples)
        keys = net.indices(prev)
        assert len(set(keys)) == 8
        net.touched.update(dict(zip(keys, entries)))
        with DE.InDomain(net):
            _a, errs, deltas = net.td_step([DE.checker(2, 1)], [prev], [1], *lr)
        assert (errs, deltas) == ([err], [delta])
        assert [net.touched[k] for k in keys] == [e + delta for e in entries]


def test_seeded_exact_rows_step_by_the_rate():
    """On the INT32_MIN row the TC step is (-2^31 * rate) >> 16 and A grows by exactly 2^31, at
    rates of 0, 1/3 and 1 and on an A of 2^62 - 2^34."""
    for lib in DE.TC_LIBS:
        bounds = DE.STAGE_BOUNDS[0] if lib in DE.STAGED_LIBS else None
        case = DE.exact_case(lib, "2x4", bounds, seed=4, ea="seeded")
        ref = DE.RefSide(case, lib)
        ref.step(case.calls[0])
        row, want, ea = case.rows[0][0], ref.want_lut(), ref.want_ea()
        s = () if bounds is None else (ref.net.stage(row.prev),)
        rates = set()
        for k, v in row.entries.items():
            e0, a0 = (int(x) for x in case.ea[(*s, *k)])
            r = TR.rate(e0, a0)
            rates.add(r)
            assert int(want[(*s, *k)]) == v + ((-(1 << 31) * r) >> 16)
            assert [int(x) for x in ea[(*s, *k)]] == [e0 - (1 << 31), a0 + (1 << 31)]
        assert {0, 21845, 65536} <= rates and int(ea[..., 1].max()) > (1 << 62) - (1 << 34)


# ------------------------------------------------------------------ the inputs pass 32 bits
def test_max_table_on_the_8x3_set_has_38_bit_values():
    lut = DE.table("max", DE.lut_shape(DE.T8M3)).numpy()
    net = NR.Net(DE.T8M3, base=lut)
    assert net.V(np.full(16, 27)) == 64 * ((1 << 31) - 1)
    low = DE.table("min", DE.lut_shape(DE.T8M3)).numpy()
    assert NR.Net(DE.T8M3, base=low).V(DE.ROW_24) == -(1 << 37)
    staged = DE.table("min", DE.lut_shape(DE.T8M3, (27,))).numpy()
    assert SR.StagedNet(DE.T8M3, (27,), base=staged).V(np.full(16, 27)) == -64 * ((1 << 31) - 1)


def test_sixteen_27s_gain_two_to_the_31_on_every_move():
    boards = DE.high_boards(np.random.default_rng(0), 12, 27)
    assert boards.max() == 27 and (boards[0] == 27).all()
    for a in range(4):
        after, gain = NR.E.move(boards[0], a)
        assert gain == 1 << 31 and sorted(after) == [0] * 8 + [28] * 8
    assert all(NR.E.move(boards[2], a)[0] == list(boards[2]) for a in range(4))  # terminal
    assert tuple(boards[3]) == DE.ROW_24
    assert [int((b == 0).sum()) for b in boards[4:8]] == [0, 1, 2, 3]
    q = NR.Net(DE.T8M3, base=DE.table("max", DE.lut_shape(DE.T8M3)).numpy()).policy(boards[0])[0]
    assert q == [(1 << 41) + 64 * ((1 << 31) - 1)] * 4


def test_a_search_case_has_a_chance_numerator_above_two_to_the_45():
    """Depth 3 on the all-24 board over the max table, p(4) = 0.1: the afterstate of eight 25s has
    eight empty cells of weight 10 each, and every child is worth two more merges (2^38 and about
    2^39) on top of V = 2^37."""
    net = NR.Net(DE.T8M3, base=DE.table("max", DE.lut_shape(DE.T8M3)).numpy())
    s = SRCH.Search(net, 0.1)
    after = bytes(NR.E.move(DE.high_boards(np.random.default_rng(0), 1, 24)[0], 2)[0])
    total = 0
    for c in (c for c in range(16) if after[c] == 0):
        for e, w in ((1, 9), (2, 1)):
            total += w * s.vmax(after[:c] + bytes([e]) + after[c + 1:], 2)
    assert total > 1 << 45 and s.vafter(after, 2) == total // 80


def test_a_learning_case_has_err_times_lr_num_above_two_to_the_53():
    """The all-27 board over a max table at lr = 2^16 / 2^31: err = 2^41, delta = 2^26."""
    net = NR.Net(DE.T8M3, base=DE.table("max", DE.lut_shape(DE.T8M3)).numpy())
    b = np.full(16, 27)
    _a, errs, deltas = net.td_step([b], [list(b)], [1], 1 << 16, 31)
    assert errs == [1 << 41] and deltas == [1 << 26] and abs(errs[0] << 16) > 1 << 53
    big = 0
    for name, lib, build in CASES:
        if lib == "td" and "lr65536_31" in name:
            case = build()
            _a, errs, _d, _s = DE.RefSide(case, lib).step(case.calls[0])
            big = max(big, max(abs(e) << 16 for e in errs))
    assert big > 1 << 53


def test_staged_bounds_lie_above_the_index_clamp():
    for bounds in DE.STAGE_BOUNDS:
        net = SR.StagedNet(NR.TUPLES_2x4, bounds)
        a, b = [17] + [0] * 15, [15] + [0] * 15
        assert net.indices(a) == net.indices(b) and min(bounds) > 15
    assert SR.StagedNet(NR.TUPLES_2x4, (16, 25)).stage([17] + [0] * 15) == 1
    assert SR.StagedNet(NR.TUPLES_2x4, (27,)).stage([26] * 16) == 0


def test_the_tables():
    shape = DE.lut_shape(NR.TUPLES_2x4, (16, 25))
    full = DE.table("full", shape[1:], seed=1).numpy().astype(np.int64)
    assert full.min() > DE.INT32_MIN and full.max() > (1 << 31) - (1 << 20) \
        and full.min() < -(1 << 31) + (1 << 20)
    edge = DE.table("edge_unset", shape, seed=2).numpy()
    share = (edge[1:] == DE.UNSET).mean()
    assert 0.45 < share < 0.55 and set(np.unique(edge[1:])) == {DE.UNSET, DE.UNSET + 1}
    assert (edge[0] != DE.UNSET).all()
    wide = DE.wide_table(shape[1:], 3).astype(np.int64)
    assert np.abs(wide).max() <= (1 << 31) - DE.HEADROOM and np.abs(wide).max() > 1 << 30


# ------------------------------------------------------------------ the guard
def test_in_domain_fires_on_a_wrapped_entry():
    prev = list(range(1, 17))
    for top, fires in ((DE.INT32_MAX - 8, False), (DE.INT32_MAX - 7, True)):
        net = NR.Net(((0, 1, 2, 3),))
        keys = net.indices(prev)
        # V = top - top - 8 = -8: err = 8 and, at lr = 1, delta = 8
        net.touched.update(dict(zip(keys, [top, -top, -2, -2, -1, -1, -1, -1])))
        try:
            with DE.InDomain(net):
                _a, errs, deltas = net.td_step([DE.checker(2, 1)], [prev], [1], 1, 0)
            assert not fires and net.touched[keys[0]] == DE.INT32_MAX
        except DE.OutOfDomain as e:
            assert fires and "entry" in str(e)
        assert (errs, deltas) == ([8], [8])


def test_in_domain_fires_on_a_wrapped_delta():
    net = NR.Net(((0, 1, 2, 3),), base=DE.table("max", (1, 65536)).numpy())
    with pytest.raises(DE.OutOfDomain, match="delta"):
        with DE.InDomain(net):  # err = -8 INT32_MAX at lr = 1
            net.td_step([DE.checker(2, 1)], [list(range(1, 17))], [1], 1, 0)
    assert NR.wrap32(1 << 31) == DE.INT32_MIN  # the guard put the reference's wrap32 back


def test_in_domain_fires_on_an_entry_landing_on_unset():
    net = SR.StagedNet(((0, 1, 2, 3),), (27,))
    prev = list(range(1, 17))
    keys = net.indices(prev)
    net.stages[0].update({k: 0 for k in keys})
    net.stages[0][keys[0]] = 8                       # V = 8, err = -8, delta = -8 at lr = 1
    net.stages[0][keys[1]] = DE.INT32_MIN + 8        # ... which V must then include
    net.stages[0][keys[2]] = DE.INT32_MAX - 7        # V = 8 + (INT32_MIN + 8) + (INT32_MAX - 7) = 8
    with pytest.raises(DE.OutOfDomain, match="UNSET"):
        with DE.InDomain(net):
            _a, errs, deltas = net.td_step([DE.checker(2, 1)], [prev], [1], 1, 0)
            assert (errs, deltas) == ([-8], [-8])


def test_in_domain_fires_on_e_above_a_and_on_a_too_large():
    for e, a in ((5, 3), (-4, 3), (0, 1 << 62)):
        tc = TR.TC(NR.Net(NR.TUPLES_2x4))
        with pytest.raises(DE.OutOfDomain, match="E, A"):
            with DE.InDomain(tc.net, tc):
                tc.E[(0, 1)], tc.A[(0, 1)] = e, a
    tc = TR.TC(NR.Net(NR.TUPLES_2x4))
    with DE.InDomain(tc.net, tc):
        tc.E[(0, 1)], tc.A[(0, 1)] = -3, (1 << 62) - 1


def test_in_domain_passes_an_exception_through_and_restores_wrap32():
    orig = NR.wrap32
    with pytest.raises(ZeroDivisionError):
        with DE.InDomain():
            1 // 0
    assert NR.wrap32 is orig


# ------------------------------------------------------------------ every learning case
def test_the_case_list_covers_what_the_issue_names():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    for lib in DE.LIBS:
        mine = [n for n in names if n.startswith(lib + "-")]
        assert sum("exact" in n for n in mine) >= 2
        for n in (2, 65, 129):
            for lr in DE.LRS:
                assert sum(f"wide-n{n}-lr{lr[0]}_{lr[1]}-" in m for m in mine) == 1
        assert any("seeds" in m for m in mine) == (lib in DE.TC_LIBS)
        assert any("edge_unset" in m for m in mine) == (lib in DE.STAGED_LIBS)
    assert "lam-exact-H2-s31" in names
    assert not any("4x6" in n for n in names)


@pytest.mark.parametrize("name,lib,build", CASES, ids=[c[0] for c in CASES])
def test_every_learning_case_is_in_domain_on_the_reference(name, lib, build):
    case = build()
    ref = DE.RefSide(case, lib)
    moved = False
    for call in case.calls:
        assert call.boards.max() <= 27 and max((int(np.max(h)) for hs in call.history
                                                 for h in hs), default=0) <= 27
        _acts, errs, deltas, _state = ref.step(call)  # raises OutOfDomain
        moved |= any(deltas)
        if call.lr in ((1, 0), (1 << 16, 16)):
            assert errs == deltas and any(errs)
    assert moved or call.lr == (0, 0)
    if "wide" in name and call.lr[1] == 31 or "seeds" in name:  # values of more than 32 bits
        assert max(abs(e) for e in errs) > 1 << 32
    if "seeds" in name:
        assert max(ref.tc.A.values()) >= 1 << 61
