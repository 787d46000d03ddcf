"""K1 (lmi_router, csrc/lmi_router.hip), every kernel path against float64.

Each answer is checked by oracle/lmi_oracle.py's check_router_rows: the float64
forward of the float32 weights with an a-priori bound on any float32
evaluation; no row is excused, and on the rows whose float64 top-1 gap exceeds
the bound (at least 90 % of every case, tests/test_oracle_router64.py) the
first pick and the argmax must be the float64 argmax itself.  The
probability rule's constant is lmi_oracle.ROUTER_PROB_CONST = 16 u; measured
on gfx950 it is never drawn on: over every case here the largest
|p - p64| / p64 minus the rule's other terms is -8.1 u (at 1 -> 1 -> 1, where
p = 1; -40 u and below elsewhere).  Each check prints its figure (pytest -s).

Which code each case reaches (read from lmi_router's dispatch):
  router_mfma_kernel<1>: MLP, MLP-2 .. MLP-7, c3, nav768, deep16, max at
      nq = 257 (auto), every row count, LMI_ROUTER_QG=1; nav768 under
      LMI_ROUTER_QG=4 (falls to <1> by LDS); its four-lane top-8 lists for
      R <= 8 and ARGMAX, select_classes' rank loop for R > 8
  router_mfma_kernel<2>: MLP at nq = 4100 (auto), LMI_ROUTER_QG=2
  router_mfma_kernel<4>: MLP at nq = 8200 (auto), LMI_ROUTER_QG=4
  router_kernel<32>, vec4 staging, whole rows: MLP-8, odd, c64, c65, deep12,
      MLP and MLP-5 under LMI_ROUTER_FMA=1; column blocks: MLP-4 under
      LMI_ROUTER_FMA=1; scalar staging: linear, one, misaligned MLP
  router_kernel<16> (widest layer > 576), vec4 staging in column blocks:
      wide-in-narrow, many-classes; scalar staging: wide, misaligned 768->128->122
  select_classes (the FMA kernel's, and the MFMA kernel's for R > 8): the
      wave-wide rounds for R <= 8, the rank loop for R > 8, ARGMAX
"""
import os

import numpy as np
import pytest
import torch

import lmi_oracle as O
import router_cases as RC
from li import _lib
from li.index import DeviceRouter

pytestmark = pytest.mark.gpu

KNOBS = ("LMI_ROUTER_FMA", "LMI_ROUTER_QG")


def _knobs(**env):
    for var in KNOBS:
        os.environ.pop(var, None)
    for var, val in env.items():
        os.environ[var] = str(val)
    _lib.load().lmi_config_reload()


@pytest.fixture(autouse=True)
def router_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    _knobs()
    yield
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    _lib.load().lmi_config_reload()


def _answers(router, x, Rs):
    """{R: (classes, probs)} and the argmax, as numpy."""
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).cuda()
    out = {}
    for R in Rs:
        cls, p = router.topr(xt, R, with_probs=True)
        out[R] = (cls.cpu().numpy(), p.cpu().numpy())
    am = router.argmax(xt).cpu().numpy()
    torch.cuda.synchronize()
    return out, am


def _check(c, out, am, rows=slice(None)):
    """Every answer of `out` / `am` against case c's float64 oracle (rows
    `rows` of it)."""
    l64, err, clear, top = c.l64[rows], c.err[rows], c.clear[rows], c.top64[rows]
    for R, (cls, p) in out.items():
        print(f"{c.name} R={R}: probability excess {O.router_prob_excess(cls, p, l64, err):.1f} u "
              f"(rule: {O.ROUTER_PROB_CONST})")
        assert O.check_router_rows(cls, p, l64, err, R) == [], (c.name, R)
        assert (cls[clear, 0] == top[clear]).all(), (c.name, R)
    assert O.check_router_rows(am, None, l64, err, 1) == [], c.name
    assert (am[clear] == top[clear]).all(), c.name


def _run(c, n=None, x=None, router=None):
    n = c.n if n is None else n
    router = router or DeviceRouter(c.layers)
    out, am = _answers(router, c.x[:n] if x is None else x, c.Rs())
    _check(c, out, am, slice(0, n))
    return out, am


def _same(a, b):
    (oa, ama), (ob, amb) = a, b
    assert np.array_equal(ama, amb)
    for R in oa:
        assert np.array_equal(oa[R][0], ob[R][0]), R
        assert np.array_equal(oa[R][1].view(np.uint32), ob[R][1].view(np.uint32)), R


@pytest.mark.parametrize("name", RC.TABLE)
def test_router_shape(name):
    _run(RC.case(name))


@pytest.mark.parametrize("name", ["MLP", "MLP-8"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 65])
def test_router_row_counts(name, n):
    _run(RC.case(name), n=n)


@pytest.mark.parametrize("n", [4100, 8200])
def test_router_auto_query_groups(n):
    """nq in [4096, 8192) takes router_mfma_kernel<2>, nq >= 8192 <4>."""
    _run(RC.case("MLP", n))


@pytest.mark.parametrize("n", [17, 65])
def test_router_forced_query_groups_agree_bitwise(n):
    """LMI_ROUTER_QG = 1, 2, 4 at row counts that leave whole query groups
    empty and the last one partial: a query's arithmetic does not depend on
    its group, so classes and probabilities are bitwise equal."""
    c = RC.case("MLP")
    got = []
    for qg in (1, 2, 4):
        _knobs(LMI_ROUTER_QG=qg)
        got.append(_run(c, n=n))
    _same(got[0], got[1])
    _same(got[0], got[2])


def test_router_query_groups_fall_back_by_lds():
    """768 -> 128 -> 1000 holds one query group's activations in the LDS:
    LMI_ROUTER_QG=4 runs <1> and answers the same bits."""
    c = RC.case("nav768")
    r = DeviceRouter(c.layers)
    a = _answers(r, c.x, (8, 9))
    _knobs(LMI_ROUTER_QG=4)
    _same(a, _answers(r, c.x, (8, 9)))


@pytest.mark.parametrize("name", ["MLP", "MLP-5", "MLP-4"])
def test_router_fma_kernel_at_mfma_widths(name):
    """LMI_ROUTER_FMA=1: router_kernel<32> on stacks the MFMA kernel takes by
    default (MLP-4's 512-wide rows in column blocks); both pass the checker
    and agree on the argmax of every clear row."""
    c = RC.case(name)
    r = DeviceRouter(c.layers)
    _, am_m = _run(c, router=r)
    _knobs(LMI_ROUTER_FMA=1)
    _, am_f = _run(c, router=r)
    assert (am_m[c.clear] == am_f[c.clear]).all()


@pytest.mark.parametrize("name", ["MLP", "MLP-8", "wide"])
def test_router_row_stride(name):
    """ldx > dims[0]: a column slice of a tensor 8 columns wider whose padding
    is NaN answers the bits of the contiguous copy."""
    c = RC.case(name)
    d = c.dims[0]
    wide = torch.full((c.n, d + 8), float("nan"), device="cuda")
    wide[:, :d] = torch.from_numpy(np.array(c.x)).cuda()
    view = wide[:, :d]
    assert view.stride(0) == d + 8 and not view.is_contiguous()
    r = DeviceRouter(c.layers)
    _same(_run(c, router=r), _run(c, x=view, router=r))


@pytest.mark.parametrize("name", ["MLP", "mis768"])
def test_router_misaligned_weights(name):
    """Weight matrices at a 4-byte offset into a flat buffer: not 16-B aligned,
    so the stack takes the FMA kernel with scalar staging."""
    c = RC.case(name)
    layers, keep = [], []
    for w, b in c.layers:
        flat = torch.zeros(w.size + 1, device="cuda")
        flat[1:] = torch.from_numpy(w.reshape(-1)).cuda()
        keep.append(flat)
        layers.append((flat[1:].view(w.shape), torch.from_numpy(b).cuda()))
    r = DeviceRouter(layers)
    for (w, _), rw in zip(layers, r.W):
        assert rw.data_ptr() == w.data_ptr() and rw.data_ptr() % 16 == 4
    _run(c, router=r)


def _tie_layers(C, seed):
    """32 -> 16 -> C whose last layer's rows and biases are duplicated in
    pairs: class 2j + 1 is a copy of class 2j (an odd C leaves the last alone)."""
    l0, l1 = RC.make_layers((32, 16, C), seed)
    w, b = l1[0].copy(), l1[1].copy()
    w[1::2] = w[0:2 * (C // 2):2]
    b[1::2] = b[0:2 * (C // 2):2]
    return [l0, (w, b)]


@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("nc", [5, 64, 65, 122])
def test_router_exact_ties(nc, fma):
    """Ties go to the lower class index, exactly, in both kernels."""
    if fma:
        _knobs(LMI_ROUTER_FMA=1)
    Rs = sorted({1, min(8, nc), min(9, nc), nc})
    # every class ties: all-zero rows through one Linear with a constant bias
    w = RC.make_layers((32, nc), 7)[0][0]
    r = DeviceRouter([(w, np.full(nc, 0.25, np.float32))])
    out, am = _answers(r, np.zeros((65, 32), np.float32), Rs)
    assert (am == 0).all()
    for R in Rs:
        cls, p = out[R]
        assert (cls == np.arange(R)[None, :]).all(), R
        assert (p == np.float32(1) / np.float32(nc)).all(), R
    # duplicated pairs: the even class directly precedes its copy
    x = RC.make_rows(65, 32, 11)
    layers = _tie_layers(nc, 13)
    out, am = _answers(DeviceRouter(layers), x, Rs)
    l64, err = O.mlp_forward64(x, layers)
    paired = 2 * (nc // 2)
    for R in Rs:
        cls, p = out[R]
        assert O.check_router_rows(cls, p, l64, err, R) == [], R
        odd = (cls % 2 == 1)
        assert not odd[:, 0].any(), R
        assert (cls[:, :-1][odd[:, 1:]] == cls[:, 1:][odd[:, 1:]] - 1).all(), R
        even = (cls % 2 == 0) & (cls < paired - 1)
        nxt = even[:, :-1]
        assert (cls[:, 1:][nxt] == cls[:, :-1][nxt] + 1).all(), R
        assert (p[:, 1:][nxt].view(np.uint32) == p[:, :-1][nxt].view(np.uint32)).all(), R
    assert (am == out[Rs[0]][0][:, 0]).all() and ((am % 2 == 0) | (am >= paired)).all()


@pytest.mark.parametrize("fma", [0, 1])
def test_router_large_logits(fma):
    """The last layer scaled by 1e4: probabilities stay finite (none NaN), the
    picks pass the checker and the top probability its rule."""
    if fma:
        _knobs(LMI_ROUTER_FMA=1)
    c = RC.case("MLP")
    (w, b) = c.layers[-1]
    layers = list(c.layers[:-1]) + [(w * np.float32(1e4), b * np.float32(1e4))]
    l64, err = O.mlp_forward64(c.x, layers)
    out, am = _answers(DeviceRouter(layers), c.x, c.Rs())
    for R, (cls, p) in out.items():
        assert np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all(), R
        assert O.check_router_rows(cls, p, l64, err, R, prob_cols=[0]) == [], R
    assert O.check_router_rows(am, None, l64, err, 1) == []


def test_neural_network_predicts_a_stack_the_fma_kernel_used_to_refuse():
    """NeuralNetwork(input_dim=768, model_type="MLP-8") (768 -> 8 -> C, not
    MFMA-eligible and wider than the old whole-row stage): predict and
    predict_proba answer through K1 and pass the checker."""
    from li.model import NeuralNetwork
    torch.manual_seed(3)
    nn = NeuralNetwork(input_dim=768, output_dim=1000, model_type="MLP-8")
    layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy())
              for m in nn.model.layers if isinstance(m, torch.nn.Linear)]
    assert [w.shape for w, _ in layers] == [(8, 768), (1000, 8)]
    x = RC.make_rows(65, 768, 5)
    l64, err = O.mlp_forward64(x, layers)
    am = nn.predict(torch.from_numpy(x))
    assert O.check_router_rows(am, None, l64, err, 1) == []
    p, cls = nn.predict_proba(torch.from_numpy(x))
    assert O.check_router_rows(cls, p, l64, err, 1000) == []
