"""The router checker (oracle/lmi_oracle.py: mlp_forward64, check_router_rows)
has teeth and accepts what it must, on the CPU: it accepts torch's float32
forward and a sequential float32 FMA chain at every shape the device tests
run, rejects four sabotaged answers, and the inputs leave at least 90 % of
the rows of every shape with a top-1 gap above the bound (on those rows the
device tests require the float64 argmax itself)."""
import numpy as np
import pytest

import lmi_oracle as O
import router_cases as RC

ALL = list(RC.SHAPES)
# a sabotaged forward shows in classes or probabilities only when there is
# more than one class, and a ReLU only exists between two Linear layers
MULTI = [k for k in ALL if RC.SHAPES[k][-1] > 1]
HIDDEN = [k for k in MULTI if len(RC.SHAPES[k]) > 2]
# How much of the forward a sabotage removes: one term or unit, except at
# 1024 -> 1024 -> 3.  There the bound (4.3e-4: two layers of (1024 + 2) u) is
# as large as what one term of 1024 moves a logit by (at most 8.9e-4, under
# the probability rule's 2 max e), so the checker can only be asked to see
# four of them (one float4 of a row, one k step of the MFMA): 1.9e-3.
SABOTAGED = {"max": 4}


def _check_logits(c, logits32):
    bad = []
    for R in c.Rs():
        cls, p = RC.answer32(logits32, R)
        bad += O.check_router_rows(cls, p, c.l64, c.err, R)
    return bad


@pytest.mark.parametrize("name", ALL)
def test_accepts_torch_float32(name):
    c = RC.case(name)
    l32 = RC.torch32_forward(c.x, c.layers)
    assert (np.abs(l32 - c.l64) <= c.err).all()
    assert _check_logits(c, l32) == []
    am = l32.argmax(axis=1)
    assert (am[c.clear] == c.top64[c.clear]).all()


@pytest.mark.parametrize("name", [k for k in ALL if max(RC.SHAPES[k]) <= 300])
def test_accepts_sequential_fma_chain(name):
    c = RC.case(name)
    l32 = RC.chain32_forward(c.x, c.layers)
    assert (np.abs(l32 - c.l64) <= c.err).all()
    assert _check_logits(c, l32) == []
    assert (l32.argmax(axis=1)[c.clear] == c.top64[c.clear]).all()


@pytest.mark.parametrize("name", ALL)
def test_most_rows_have_a_clear_top1(name):
    c = RC.case(name)
    assert c.clear.mean() >= 0.90


@pytest.mark.parametrize("name", MULTI)
def test_rejects_a_dropped_input_column(name):
    c = RC.case(name)
    w0, b0 = c.layers[0]
    nd = SABOTAGED.get(name, 1)
    l32 = RC.torch32_forward(c.x[:, :-nd], [(w0[:, :-nd], b0)] + list(c.layers[1:]))
    assert _check_logits(c, l32) != []


@pytest.mark.parametrize("name", HIDDEN)
def test_rejects_a_missing_relu(name):
    """One hidden unit of the first hidden layer without its ReLU: the unit
    whose negative pre-activations weigh most."""
    c = RC.case(name)
    w0, b0 = c.layers[0]
    z = c.x.astype(np.float64) @ w0.astype(np.float64).T + b0
    unit = np.argsort(np.minimum(z, 0).sum(axis=0))[:SABOTAGED.get(name, 1)]
    h = RC.torch32_forward(c.x, [c.layers[0]])
    h1 = np.maximum(h, 0)
    h1[:, unit] = h[:, unit]
    rest = list(c.layers[1:])
    if len(rest) > 1:
        # the hidden layers after it keep their ReLU
        h2 = np.maximum(RC.torch32_forward(h1, [rest[0]]), 0)
        l32 = RC.torch32_forward(h2, rest[1:])
    else:
        l32 = RC.torch32_forward(h1, rest)
    assert _check_logits(c, l32) != []


@pytest.mark.parametrize("name", MULTI)
def test_rejects_swapped_picks(name):
    """Two consecutive picks swapped across a gap larger than the bound:
    exactly that row fails."""
    c = RC.case(name)
    R = c.C
    cls = O.rank_classes(c.l64)[:, :R].copy()
    rows = np.arange(c.n)[:, None]
    gap = (c.l64[rows, cls[:, :-1]] - c.err[rows, cls[:, :-1]]) - \
          (c.l64[rows, cls[:, 1:]] + c.err[rows, cls[:, 1:]])
    assert O.check_router_rows(cls, None, c.l64, c.err, R) == []
    i, r = np.unravel_index(gap.argmax(), gap.shape)
    assert gap[i, r] > 0
    cls[i, r], cls[i, r + 1] = cls[i, r + 1], cls[i, r]
    assert O.check_router_rows(cls, None, c.l64, c.err, R) == [(int(i), "picks out of order")]
    # and a clear winner left out of the top 1
    top = O.rank_classes(c.l64)[:, :2]
    bad = O.check_router_rows(top[:, 1:], None, c.l64, c.err, 1)
    assert sorted(r for r, _ in bad) == list(np.nonzero(c.clear)[0])


@pytest.mark.parametrize("name", MULTI)
def test_rejects_probabilities_normalised_over_fewer_classes(name):
    c = RC.case(name)
    l32 = RC.torch32_forward(c.x, c.layers)
    z = np.exp(l32 - l32.max(axis=1, keepdims=True))
    p = (z / np.sort(z, axis=1)[:, 1:].sum(axis=1, keepdims=True)).astype(np.float32)  # C - 1 of them
    cls = O.rank_classes(l32)
    bad = O.check_router_rows(cls, np.take_along_axis(p, cls, axis=1), c.l64, c.err, c.C)
    assert len(bad) == c.n and {r for _, r in bad} == {"probability off"}


def test_rejects_malformed_picks():
    c = RC.case("odd")
    cls = O.rank_classes(c.l64)[:, :3].copy()
    cls[4, 1] = cls[4, 0]
    cls[9, 2] = c.C
    cls[11, 0] = -1
    bad = O.check_router_rows(cls, None, c.l64, c.err, 3)
    assert {(4, "repeated class"), (9, "class out of range"), (11, "class out of range")} <= set(bad)
    assert {r for r, _ in bad} == {4, 9, 11}
    p = np.full((c.n, 3), np.nan, np.float32)
    assert len(O.check_router_rows(O.rank_classes(c.l64)[:, :3], p, c.l64, c.err, 3)) == c.n
