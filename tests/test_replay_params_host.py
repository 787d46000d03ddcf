"""The host replay (lmi_replay / lmi_replay_f64, C++) against the numpy oracle
(O.replay) off k_round = 10: bit for bit in distances and ids over k_round
1 .. 32, R 1 .. 5, float32 and float64 lists, thresholds on and off, k_final
1 .. 2 k_round, k_list = k_round and beyond, and R = 1 with threshold_dist.
The device replay's parameter tests (test_gpu_replay_params.py) compare
against this twin, so it is pinned here first, on the CPU."""
import numpy as np
import pytest

import lmi_oracle as O
import replay_cases as RC
from li import _lib
from li.index import replay

NQ, C = 300, 12
KRS = {"<=10": (1, 2, 5, 8, 9), "11-16": (11, 16), "17-32": (17, 31, 32)}


def _lists(seed, R, kr, k_list, dtype):
    # buckets of 1 and k_round - 1 rows, an empty one, and probes of it
    lists = RC.make_lists(seed, NQ, R, C, k_list, dtype, sized={2: 1, 7: kr - 1}, empty=(4,),
                          probe_empty=True)
    RC.check_sorted(lists[1], lists[2])
    return lists


def _both(classes, d, pos, size, ids, stats, **kw):
    ref_d, ref_a = O.replay(classes, d, pos, bucket_size=size, pos_to_id=ids, stats=stats, **kw)
    got_d, got_a = replay(classes, d, pos, bucket_size=size, pos_to_id=ids, **kw)
    assert got_d.dtype == np.float64 and got_a.dtype == np.uint32
    np.testing.assert_array_equal(got_d, ref_d, err_msg=str(kw))
    np.testing.assert_array_equal(got_a, ref_a, err_msg=str(kw))


@pytest.mark.parametrize("cls", list(KRS))
def test_host_replay_equals_oracle_over_the_parameter_space(cls):
    """Every k_round of one membership class of the device kernel (fill<10>,
    <16>, <32>): all four of the oracle's branch counters must be hit
    somewhere in the class, so the quirk paths run on rows of that width."""
    stats = {}
    for kr in KRS[cls]:
        assert RC.kr_class(kr) == cls
        for R in (1, 2, 3, 5):
            for dtype in (np.float32, np.float64):
                for thr in ((False,) if R == 1 else (True, False)):
                    k_list = kr + (6 if (R + thr + (dtype == np.float64)) % 2 else 0)
                    lists = _lists(1000 * kr + 10 * R + thr, R, kr, k_list, dtype)
                    for k_final in RC.k_finals(kr, R):
                        _both(*lists, stats, k_round=kr, k_final=k_final, use_threshold=thr)
                    if R > 1:  # one more k_final inside [1, 2 kr], by the seed
                        k_final = 1 + (7 * kr + 3 * R + thr) % min(RC.MAX_K, 2 * kr)
                        _both(*lists, stats, k_round=kr, k_final=k_final, use_threshold=thr)
        # R = 1 with threshold_dist: none, a few and most entries relevant
        for dtype in (np.float32, np.float64):
            for k_list in (kr, kr + 6):
                lists = _lists(77 * kr + k_list, 1, kr, k_list, dtype)
                thr0 = np.random.default_rng(kr).choice([0.1, 0.25, 0.5, 0.9], NQ)
                _both(*lists, stats, k_round=kr, k_final=kr, use_threshold=False, thr_round0=thr0)
    for key in ("quirk0", "quirk_thr", "skipped", "fillers"):
        assert stats[key] > 0, (cls, stats)


@pytest.mark.parametrize("kr,R,k_final", [(5, 2, 11), (16, 3, 33), (32, 2, 65), (1, 4, 3)])
def test_illegal_k_final_is_refused_by_both(kr, R, k_final):
    """k_final above 2 k_round fails the reference's assert at the first merge
    (LearnedIndex.py:99): the oracle asserts, lmi_replay returns
    LMI_E_INVALID."""
    classes, d, pos, size, ids = _lists(5, R, kr, kr, np.float32)
    kw = dict(k_round=kr, k_final=k_final, bucket_size=size, pos_to_id=ids, use_threshold=True)
    with pytest.raises(AssertionError):
        O.replay(classes, d, pos, **kw)
    with pytest.raises(_lib.LmiError) as e:
        replay(classes, d, pos, **kw)
    assert e.value.rc == _lib.LMI_E_INVALID
