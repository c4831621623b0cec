"""Without a GPU: the sequences of tests/lane_hot_cases.py hold what tests/test_gpu_lane_hot.py is about. On the CPU oracle every
new-vectors step of the steady-state sequence has members that change no working set and members that change it (the one exception:
1 x 2 at a perturbation of 0.02, where nothing changes), and the 1 x 2 batch carries members whose previous QP ended infeasible."""
import pytest

import lane_hot_cases as C

# (members without, with) a working-set change in the first new-vectors step
FIRST_STEP = {0.3: ((24, 126), (71, 79), (34, 116), (31, 119), (141, 9)), 0.02: ((127, 23), (143, 7), (141, 9), (139, 11), (150, 0))}


@pytest.mark.parametrize("rel", C.RELS)
def test_every_step_mixes_members_with_and_without_a_change(oracle, rel):
    for shape, first in zip(C.SHAPES, FIRST_STEP[rel]):
        rows = C.steady_oracle(oracle, shape, rel)
        assert C.changes(rows[1]) == first, (shape, C.changes(rows[1]))
        for k, kind in enumerate(C.KINDS):
            if kind == "vectors" and (shape, rel) != ((1, 2), 0.02):
                without, with_ = C.changes(rows[k])
                assert without > 0 and with_ > 0, (shape, k)
    # members that hot-start from a QP that ended infeasible
    rows = C.steady_oracle(oracle, (1, 2), 0.3)
    assert [sum(a.infeasible for a in r) for r in rows[:2]] == [8, 70]


def test_patterns_of_their_own(oracle):
    rows = C.own_pattern_oracle(oracle)
    for k, kind in enumerate(C.KINDS):
        if kind == "vectors":
            without, with_ = C.changes(rows[k])
            assert without > 0 and with_ > 0, k
