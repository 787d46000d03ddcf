"""The host side of the minibatch training mode, without a device: argument
validation of lmi_mlp_train_steps / lmi_mlp_train_workspace_bytes, the
ValueErrors of NeuralNetwork.train_minibatch and LearnedIndex.build, and the
command line's --train-mode."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from li import _lib
from li.LearnedIndex import LearnedIndex
from li.model import NeuralNetwork

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000  # a non-null "device pointer" that validation never dereferences


def _desc(dims, null=None):
    d = _lib.MlpTrainDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims[:_lib.LMI_MAX_LAYERS + 1]):
        d.dims[i] = v
    for i in range(min(d.n_layers, _lib.LMI_MAX_LAYERS)):
        for name in ("W", "b", "W_exp_avg", "W_exp_avg_sq", "b_exp_avg", "b_exp_avg_sq"):
            getattr(d, name)[i] = 0 if null == (name, i) else FAKE
    return d


def _steps(desc, **kw):
    a = dict(x=FAKE, n=1000, ldx=96, y=FAKE, order=FAKE, n_order=1000, batch=256, first_step=0,
             n_steps=1, adam_t0=0, loss=FAKE, ws=FAKE, ws_bytes=1 << 30)
    a.update(kw)
    lib = _lib.load()
    rc = lib.lmi_mlp_train_steps(C.byref(desc) if desc is not None else None, a["x"], a["n"], a["ldx"],
                                 a["y"], a["order"], a["n_order"], a["batch"], a["first_step"],
                                 a["n_steps"], a["adam_t0"], 0.01, 0.9, 0.999, 1e-8, a["loss"], a["ws"],
                                 a["ws_bytes"], None)
    return rc, lib.lmi_last_error().decode()


GOOD = (96, 256, 128, 122)


@pytest.mark.parametrize("kw,word", [
    (dict(x=0), "null"), (dict(y=0), "null"), (dict(order=0), "null"), (dict(loss=0), "null"),
    (dict(ws=0), "null"),
    (dict(batch=0), "batch < 1"),
    (dict(ldx=95), "ldx"),
    (dict(first_step=4), "first_step"),          # 4 * 256 >= 1000
    (dict(first_step=3, n_steps=2), "past the end"),
])
def test_invalid_step_arguments(kw, word):
    rc, msg = _steps(_desc(GOOD), **kw)
    assert rc == _lib.LMI_E_INVALID and word in msg, (rc, msg)


def test_invalid_descriptors():
    rc, msg = _steps(None)
    assert rc == _lib.LMI_E_INVALID and "null" in msg
    for dims in ((96,), tuple([16] * (_lib.LMI_MAX_LAYERS + 2))):
        d = _desc(dims)
        rc, msg = _steps(d)
        assert rc == _lib.LMI_E_INVALID and "n_layers" in msg, (dims, rc, msg)
        assert _lib.load().lmi_mlp_train_workspace_bytes(C.byref(d), 256) == 0
    for dims in ((96, _lib.LMI_TRAIN_MAX_DIM + 1, 10), (96, 0, 10)):
        rc, msg = _steps(_desc(dims))
        assert rc == _lib.LMI_E_INVALID and "dims[1]" in msg, (dims, rc, msg)
    rc, msg = _steps(_desc(GOOD, null=("b_exp_avg_sq", 2)))
    assert rc == _lib.LMI_E_INVALID and "layer 2" in msg, (rc, msg)


def test_small_workspace_is_refused():
    d = _desc(GOOD)
    need = _lib.load().lmi_mlp_train_workspace_bytes(C.byref(d), 256)
    rc, msg = _steps(d, ws_bytes=need - 1)
    assert rc == _lib.LMI_E_WORKSPACE and "workspace" in msg
    # the last step of the pass, with exactly the workspace asked for: nothing to refuse before the
    # launch itself (n_steps = 0 launches nothing)
    rc, msg = _steps(d, ws_bytes=need, first_step=3, n_steps=0)
    assert rc == _lib.LMI_OK


def test_workspace_grows_with_batch_and_widths():
    ws = lambda dims, batch: _lib.load().lmi_mlp_train_workspace_bytes(C.byref(_desc(dims)), batch)
    assert 0 < ws(GOOD, 1) == ws(GOOD, 16) < ws(GOOD, 17) < ws(GOOD, 256) < ws(GOOD, 1024)
    assert ws((96, 128, 122), 256) < ws((96, 256, 122), 256) < ws((96, 256, 128, 122), 256)
    assert ws((20, 8, 5), 256) < ws((768, 32, 10), 256)
    # every activation and delta of a 256-row minibatch fits: (96 + 256 + 128) + (256 + 128 + 128)
    # padded floats per row, and the per-row losses
    assert ws(GOOD, 256) >= 4 * 256 * (96 + 256 + 128 + 256 + 128 + 122 + 1)
    assert ws(GOOD, 0) == 0


def test_build_refuses_an_unknown_train_mode():
    df = pd.DataFrame(np.zeros((8, 4), dtype=np.float32))
    df.index += 1
    with pytest.raises(ValueError, match="train_mode"):
        LearnedIndex().build(df, n_categories=2, epochs=1, train_mode="bogus")


def _xy(d=12, c=5, n=32):
    return torch.zeros(n, d), torch.zeros(n, dtype=torch.long)


def test_train_minibatch_refuses_what_the_kernel_does_not_compute():
    X, Y = _xy()
    mk = lambda **kw: NeuralNetwork(input_dim=12, output_dim=5, lr=0.01, **kw)
    with pytest.raises(ValueError, match="class_weight"):
        mk(class_weight=torch.ones(5)).train_minibatch(X, Y)
    with pytest.raises(ValueError, match="CrossEntropyLoss"):
        mk(loss=torch.nn.MultiMarginLoss).train_minibatch(X, Y)
    nn = mk()
    nn.optimizer = torch.optim.SGD(nn.model.parameters(), lr=0.01)
    with pytest.raises(ValueError, match="Adam"):
        nn.train_minibatch(X, Y)
    for kw in (dict(betas=(0.8, 0.999)), dict(eps=1e-6), dict(weight_decay=0.1), dict(amsgrad=True)):
        nn = mk()
        nn.optimizer = torch.optim.Adam(nn.model.parameters(), lr=0.01, **kw)
        with pytest.raises(ValueError, match="default hyperparameters"):
            nn.train_minibatch(X, Y)
    with pytest.raises(ValueError, match="MLP-9"):
        mk(model_type="MLP-9").train_minibatch(X, Y)
    wide = NeuralNetwork(input_dim=_lib.LMI_TRAIN_MAX_DIM + 1, output_dim=5, lr=0.01)
    with pytest.raises(ValueError, match="LMI_TRAIN_MAX_DIM"):
        wide.train_minibatch(torch.zeros(4, _lib.LMI_TRAIN_MAX_DIM + 1), torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="label"):
        mk().train_minibatch(X, Y + 5)
    with pytest.raises(ValueError, match="data_X"):
        mk().train_minibatch(torch.zeros(32, 11), Y)


def test_train_minibatch_has_no_cpu_fallback():
    X, Y = _xy()
    nn = NeuralNetwork(input_dim=12, output_dim=5, lr=0.01)
    nn.model.cpu()                      # (in place: the optimizer keeps its parameters)
    nn.device = torch.device("cpu")
    before = [p.detach().clone() for p in nn.model.parameters()]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nn.train_minibatch(X, Y)
    assert all(torch.equal(a, b) for a, b in zip(before, nn.model.parameters()))
    assert len(nn.optimizer.state) == 0


def test_search_cli_takes_train_mode():
    pkg = os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import search
    parser = search.build_parser()
    assert parser.parse_args([]).train_mode == "reference"
    assert parser.parse_args(["--train-mode", "minibatch"]).train_mode == "minibatch"
    with pytest.raises(SystemExit):
        parser.parse_args(["--train-mode", "bogus"])
