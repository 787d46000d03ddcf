"""The host side of adaptive probing, without a device: the stop rule restated
in numpy (li.index.probe_stop_mask) on hand-worked rows, the argument
validation of lmi_router_stop (LMI_E_INVALID before any device call), the
ValueErrors of LearnedIndex.search and Searcher.search, and the command line's
--stop-mass / --min-buckets."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from li import _lib
from li.index import Searcher, probe_stop_mask
from li.LearnedIndex import LearnedIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer" that validation never dereferences
f32 = np.float32


def _mask(row, stop, mp=1):
    return probe_stop_mask(np.array([row], dtype=f32), stop, mp)[0].tolist()


def test_rule_on_hand_worked_rows():
    # S = 0, .5, .75, .875: probe r kept iff S_r < stop
    row = [0.5, 0.25, 0.125, 0.0625]
    assert _mask(row, 0.6) == [True, True, False, False]
    assert _mask(row, 0.8) == [True, True, True, False]
    assert _mask(row, 1.0) == [True, True, True, True]
    # probe 0 is always kept (S_0 = 0 < stop for every valid stop)
    assert _mask(row, 1e-30) == [True, False, False, False]
    assert _mask([1.0, 0.0, 0.0], 0.5) == [True, False, False]
    # S_r == stop drops probe r: the comparison is strict
    assert _mask(row, 0.5) == [True, False, False, False]
    assert _mask(row, 0.75) == [True, True, False, False]
    assert _mask(row, np.nextafter(f32(0.75), f32(1))) == [True, True, True, False]
    # min_probes is honoured, and a value above R keeps everything
    assert _mask(row, 0.5, 3) == [True, True, True, False]
    assert _mask(row, 0.5, 4) == _mask(row, 0.5, 9) == [True] * 4
    assert _mask(row, 0.8, 2) == _mask(row, 0.8, 1)
    # several rows at once, each on its own
    got = probe_stop_mask(np.array([row, [0.9, 0.05, 0.03, 0.02]], f32), 0.8)
    assert got.tolist() == [[True, True, True, False], [True, False, False, False]]
    assert got.dtype == bool and got.shape == (2, 4)


def test_mask_is_a_prefix():
    rng = np.random.Generator(np.random.PCG64(5))
    p = rng.dirichlet(np.full(12, 0.3), size=500).astype(f32)
    p = -np.sort(-p, axis=1)[:, :9]
    for stop in (0.3, 0.7, 0.95, 1.0):
        for mp in (1, 2, 9):
            keep = probe_stop_mask(p, stop, mp)
            assert keep[:, 0].all() and (np.diff(keep.astype(np.int8), axis=1) <= 0).all()
            assert (keep.sum(1) >= mp).all()
    # (the rule does not need sorted probabilities to give a prefix: the sums do not decrease)
    assert (np.diff(probe_stop_mask(p[:, ::-1], 0.5).astype(np.int8), axis=1) <= 0).all()


def test_sum_is_float32_in_ascending_order():
    # float32: .5 + 2^-25 is a tie and rounds to even, .5, twice: S_3 = .5 < stop, probe 3 kept;
    # float64: S_3 = .5 + 2^-24 == stop, probe 3 dropped
    e = 2.0 ** -25
    row, stop = [0.5, e, e, 0.25], 0.5 + 2.0 ** -24
    assert f32(stop) == stop and float(np.sum(np.array(row[:3], np.float64))) == stop
    assert _mask(row, stop) == [True, True, True, True]
    # ascending r: the small terms first add up (2^-25 + 2^-25 = 2^-24, then + .5 exactly):
    # S_3 == stop, dropped -- a descending or pairwise sum of the first row would decide otherwise
    assert _mask([e, e, 0.5, 0.25], stop) == [True, True, True, False]
    # a float64 stop mass is compared as the float32 the kernel receives
    assert _mask([0.5, 0.25], 0.5 + 2.0 ** -30) == [True, False]


@pytest.mark.parametrize("bad", [0.0, -0.5, 1.5, float("nan"), float("inf"), 1e-60])
def test_mask_refuses_a_bad_stop_mass(bad):
    with pytest.raises(ValueError, match="stop_mass"):
        probe_stop_mask(np.ones((1, 2), f32), bad)


def test_mask_refuses_bad_min_probes_and_shapes():
    for mp in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_probes"):
            probe_stop_mask(np.ones((1, 2), f32), 0.5, mp)
    with pytest.raises(ValueError):
        probe_stop_mask(np.ones(3, f32), 0.5)


def test_rule_needs_no_oracle():
    import li.index
    src = open(li.index.__file__).read()
    assert "lmi_oracle" not in src and "import oracle" not in src


# ---- lmi_router_stop's argument checks ---------------------------------------
def _desc(dims=(96, 128, 122)):
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i in range(d.n_layers):
        d.W[i] = FAKE
        d.b[i] = FAKE
    return d


def _stop(desc="good", **kw):
    a = dict(x=FAKE, nq=16, ldx=96, R=4, stop_mass=0.8, min_probes=1, classes=FAKE, probs=0, n=0)
    a.update(kw)
    lib = _lib.load()
    d = _desc() if desc == "good" else desc
    rc = lib.lmi_router_stop(a["x"], a["nq"], a["ldx"], C.byref(d) if d is not None else None, a["R"],
                             a["stop_mass"], a["min_probes"], a["classes"], a["probs"], a["n"], None)
    return rc, lib.lmi_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(stop_mass=0.0), "stop_mass"), (dict(stop_mass=-0.25), "stop_mass"),
    (dict(stop_mass=1.0000001), "stop_mass"), (dict(stop_mass=float("nan")), "stop_mass"),
    (dict(stop_mass=float("inf")), "stop_mass"),
    (dict(min_probes=0), "min_probes"), (dict(min_probes=-3), "min_probes"),
    (dict(R=0), "R out of range"), (dict(R=-1), "R out of range"), (dict(R=123), "R out of range"),
    (dict(x=0), "null"), (dict(classes=0), "null"),
    (dict(nq=-1), "nq"), (dict(ldx=95), "ldx"),
])
def test_invalid_arguments(kw, word):
    rc, msg = _stop(**kw)
    assert rc == _lib.LMI_E_INVALID and word in msg, (rc, msg)


def test_invalid_descriptor_and_empty_batch():
    rc, msg = _stop(desc=None)
    assert rc == _lib.LMI_E_INVALID and "null" in msg
    d = _desc()
    d.n_layers = 0
    rc, msg = _stop(desc=d)
    assert rc == _lib.LMI_E_INVALID and "n_layers" in msg
    rc, msg = _stop(desc=_desc((96, _lib.LMI_ROUTER_MAX_DIM + 1, 10)))
    assert rc == _lib.LMI_E_UNSUPPORTED
    # nothing to route: no device call, valid arguments
    assert _stop(nq=0)[0] == _lib.LMI_OK
    assert _stop(nq=0, stop_mass=1.0, min_probes=99, R=122)[0] == _lib.LMI_OK
    assert "lmi_router_stop" in _lib.EXPORTS and _lib.LMI_PROBE_NONE == -1
    assert _lib.load().lmi_abi_version() == 13


# ---- the Python layers refuse the same values before any device call ----------
BAD = [dict(stop_mass=0.0), dict(stop_mass=-1.0), dict(stop_mass=1.5), dict(stop_mass=float("nan")),
       dict(stop_mass=0.8, min_probes=0)]


@pytest.mark.parametrize("kw", BAD)
def test_searcher_refuses_bad_rule(kw):
    s = Searcher(None, None, exchange=False)   # (no index, no router: nothing to touch)
    for call in (lambda: s.search(None, None, 4, **kw), lambda: s.route(None, 4, **kw),
                 lambda: s.lists(None, None, 4, 10, **kw), lambda: s.streamed(None, None, 4, **kw),
                 lambda: s.graph(None, None, 4, **kw)):
        with pytest.raises(ValueError, match="stop_mass|min_probes"):
            call()


@pytest.mark.parametrize("kw", BAD)
def test_learned_index_refuses_bad_rule(kw):
    kw = {("min_buckets" if k == "min_probes" else k): v for k, v in kw.items()}
    with pytest.raises(ValueError, match="stop_mass|min_probes"):
        LearnedIndex().search(None, None, None, None, None, n_buckets=4, **kw)


def test_search_cli_takes_the_two_flags():
    pkg = os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import search
    parser = search.build_parser()
    a = parser.parse_args([])
    assert a.stop_mass is None and a.min_buckets == 1
    a = parser.parse_args(["--stop-mass", "0.9", "--min-buckets", "2"])
    assert a.stop_mass == 0.9 and a.min_buckets == 2
    with pytest.raises(SystemExit):
        parser.parse_args(["--stop-mass", "much"])
    # the result file's name: unchanged without the flag
    ident = search.result_identifier("pca96v2", "10M", 205, 0.009, 122, "MLP-5", 4)
    assert ident == "learned-index-pca96v2-10M-ep=205-lr=0.009-cat=122-model=MLP-5-buck=4"
    assert search.result_identifier("pca96v2", "10M", 205, 0.009, 122, "MLP-5", 4, 0.9) == ident + "-stop=0.9"
    with pytest.raises(ValueError, match="stop_mass"):
        search.run("pca96v2", "pca96", n_buckets_perc=[4], n_categories=122, stop_mass=2.0)
