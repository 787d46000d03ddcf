"""Drop-in for the reference's search/li/model.py with inference on K1.

Same names, architectures and return types as the reference:

  Model            model.py:15-83   nn.Sequential 'layers' of Linear/ReLU per
                                     model_type ('MLP' ... 'MLP-9')
  data_X_to_torch  model.py:86-89
  data_to_torch    model.py:92-96
  get_device       model.py:99-111
  NeuralNetwork    model.py:114-229  train unchanged (torch); train_batch
                                     computes only the minibatch the reference's
                                     loop uses (each epoch's last), bitwise its
                                     result; LMI_TRAIN_VERBATIM=1: its loop,
                                     predict / predict_proba on the GPU router
                                     kernel (lmi_router, liblmi_hip.so);
                                     train_minibatch (not in the reference):
                                     an Adam step on EVERY minibatch, on the
                                     fused training kernels (K6, lmi_train)
  LIDataset        model.py:232-240  (1-based __getitem__, as the reference)

predict_proba returns (probs f32 ndarray, classes int64 ndarray), both
(n, n_classes), classes by descending probability (ties to the lower class),
like `softmax(outputs, dim=1).topk(C)` (model.py:220-227).  predict returns
argmax labels (int64), like `torch.max(outputs, 1)` (model.py:207-211).
There is no CPU fallback: on a host without a HIP device these raise.
"""
from __future__ import annotations

import os
from typing import Tuple

import numpy as np
import torch
import torch.utils.data

from .Logger import Logger

torch.manual_seed(2023)
np.random.seed(2023)

_ARCH = {
    "MLP": (128,), "MLP-2": (64,), "MLP-3": (256,), "MLP-4": (512,), "MLP-5": (256, 128),
    "MLP-6": (32,), "MLP-7": (16,), "MLP-8": (8,),
}


class Model(torch.nn.Module):
    """The model class representing the index (model.py:15-83)."""

    def __init__(self, input_dim=768, output_dim=1000, model_type=None):
        super().__init__()
        if model_type in _ARCH:
            dims = [input_dim, *_ARCH[model_type], output_dim]
            mods = []
            for i, (a, b) in enumerate(zip(dims, dims[1:])):
                mods.append(torch.nn.Linear(a, b))
                if i + 2 < len(dims):
                    mods.append(torch.nn.ReLU())
            self.layers = torch.nn.Sequential(*mods)
        elif model_type == "MLP-9":
            # shape-inconsistent in the reference too (model.py:71-78): the
            # second Linear expects input_dim features but receives 8
            self.layers = torch.nn.Sequential(
                torch.nn.Linear(input_dim, 8), torch.nn.ReLU(),
                torch.nn.Linear(input_dim, 16), torch.nn.ReLU(),
                torch.nn.Linear(16, output_dim))
        self.n_output_neurons = output_dim

    def forward(self, x: torch.FloatTensor) -> torch.FloatTensor:
        return self.layers(x)


def data_X_to_torch(data) -> torch.FloatTensor:
    """Creates torch training data (model.py:86-89)."""
    return torch.from_numpy(np.array(data).astype(np.float32))


def data_to_torch(data, labels) -> Tuple[torch.FloatTensor, torch.LongTensor]:
    data_X = data_X_to_torch(data)
    data_y = torch.as_tensor(torch.from_numpy(labels), dtype=torch.long)
    return data_X, data_y


def get_device() -> torch.device:
    """model.py:99-111 (cuda:0 there): the process's current device, which is
    cuda:0 in one process and the rank's own GPU under a launcher."""
    use_cuda = torch.cuda.is_available()
    device = torch.device("cuda", torch.cuda.current_device()) if use_cuda else torch.device("cpu")
    torch.backends.cudnn.benchmark = True
    return device


def last_batch_indices(indices: torch.Tensor, batch_size: int, loader_gen=None,
                       sampler_gen=None) -> torch.Tensor:
    """The dataset ids of the LAST minibatch of one pass over
    DataLoader(ds, batch_size, sampler=SubsetRandomSampler(indices)), drawn as
    iter(DataLoader) draws them: first the iterator's base seed from the
    loader's generator (one int64 `random_`), then the sampler's
    `randperm(len(indices))` from the sampler's generator (None: the global CPU
    generator); the pass's last batch is the permutation's last
    `n % batch_size or batch_size` entries, in order."""
    n = indices.shape[0]
    torch.empty((), dtype=torch.int64).random_(generator=loader_gen)
    perm = torch.randperm(n, generator=sampler_gen)
    return indices[perm[n - (n % batch_size or batch_size):]] if n else indices[:0]


class NeuralNetwork(Logger):
    """The router (model.py:114-229); inference runs on K1 (lmi_router)."""

    # class-level defaults: an instance unpickled from the reference's own
    # pickle (li.index_io.load_index) carries only the reference's attributes
    _router = None
    _router_version = None

    def __init__(self, input_dim, output_dim, loss=torch.nn.CrossEntropyLoss, lr=0.1,
                 model_type="MLP", class_weight=None):
        self.device = get_device()
        self.model = Model(input_dim, output_dim, model_type=model_type).to(self.device)
        if class_weight is not None:
            self.loss = loss(weight=class_weight.to(self.device))
        else:
            self.loss = loss()
        self.optimizer = torch.optim.Adam(self.model.parameters(), lr=lr)
        self._router = None
        self._router_version = None

    def __getstate__(self):
        """Pickle what the reference pickles: the device router (ctypes
        descriptors over HBM) is rebuilt from the weights after loading."""
        st = dict(self.__dict__)
        st.pop("_router", None)
        st.pop("_router_version", None)
        return st

    # ---- training (index build; unchanged semantics, torch) ----------------
    def train(self, data_X, data_y, epochs=500, logger=None):
        step = epochs // 10
        losses = []
        if logger:
            logger.info(f"Epochs: {epochs}, step: {step}")
        for ep in range(epochs):
            pred_y = self.model(data_X.to(self.device))
            curr_loss = self.loss(pred_y, data_y.to(self.device))
            if ep % step == 0 and ep != 0 and logger:
                logger.info(f"Epoch {ep} | Loss {curr_loss.item()}")
            losses.append(curr_loss.item())
            self.model.zero_grad()
            curr_loss.backward()
            self.optimizer.step()
        return losses

    def _last_batch_plan(self, loader):
        """(dataset, indices LongTensor, batch size) when `loader` is the
        build's kind of DataLoader (LearnedIndex.build) and the model is made of
        Linear and ReLU only, so that the forwards train_batch throws away have
        no effect on the weights; None otherwise (the verbatim loop runs)."""
        D = torch.utils.data
        if os.environ.get("LMI_TRAIN_VERBATIM") == "1" or type(loader) is not D.DataLoader:
            return None
        ds, sampler = loader.dataset, loader.sampler
        if (loader.num_workers != 0 or type(loader.batch_sampler) is not D.BatchSampler
                or loader.batch_sampler.sampler is not sampler or loader.drop_last
                or not loader.batch_size or loader.collate_fn is not D.default_collate
                or type(sampler) is not D.SubsetRandomSampler
                or not isinstance(ds, LIDataset) or type(ds).__getitem__ is not LIDataset.__getitem__
                or hasattr(ds, "__getitems__") or len(sampler.indices) == 0):
            return None
        leaves = [m for m in self.model.modules() if not list(m.children())]
        if not leaves or not all(type(m) in (torch.nn.Linear, torch.nn.ReLU) for m in leaves):
            return None
        try:
            indices = torch.as_tensor(sampler.indices, dtype=torch.int64)
        except (TypeError, ValueError, RuntimeError):
            return None
        return (ds, indices, int(loader.batch_size)) if indices.dim() == 1 else None

    def train_batch(self, dataset, epochs=5, logger=None):
        """model.py:174-199, including its behaviour of stepping once per
        epoch on the last minibatch's loss.

        The reference runs a forward over every minibatch of the loader and
        uses only the last one's loss.  For the loader LearnedIndex.build makes
        (see _last_batch_plan) an epoch here computes that last minibatch alone:
        the same draws from the same generators (last_batch_indices), the same
        rows, one forward -- bitwise the reference loop's weights, losses and
        final RNG state (tests/test_train_fast.py).  Any other argument, or
        LMI_TRAIN_VERBATIM=1, runs the reference's loop as it is."""
        step = max(epochs // 10, 1)
        losses = []
        if logger:
            logger.info(f"Epochs: {epochs}, step: {step}")
        plan = self._last_batch_plan(dataset)
        for ep in range(epochs):
            if plan is not None:
                ds, indices, batch_size = plan
                idx = last_batch_indices(indices, batch_size, dataset.generator,
                                         dataset.sampler.generator) - 1   # LIDataset.__getitem__
                pred_y = self.model(ds.dataset_x[idx].to(self.device))
                curr_loss = self.loss(pred_y, ds.dataset_y[idx].to(self.device))
            else:
                for data_X, data_y in iter(dataset):
                    pred_y = self.model(data_X.to(self.device))
                    curr_loss = self.loss(pred_y, data_y.to(self.device))
            if ep % step == 0 and ep != 0 and logger:
                logger.info(f"Epoch {ep} | Loss {curr_loss.item():.5f}")
            losses.append(curr_loss.item())
            self.model.zero_grad()
            curr_loss.backward()
            self.optimizer.step()
        return losses

    # ---- training that steps on every minibatch (K6) --------------------------
    def _minibatch_linears(self):
        """The model's Linear layers when train_minibatch's kernels compute
        exactly what torch would for this object's model, loss and optimizer;
        ValueError otherwise (there is no torch fallback)."""
        from . import _lib
        loss = self.loss
        if type(loss) is not torch.nn.CrossEntropyLoss:
            raise ValueError(f"train_minibatch needs CrossEntropyLoss(), not {type(loss).__name__}")
        if loss.weight is not None:
            raise ValueError("train_minibatch does not take a loss with class_weight")
        if loss.reduction != "mean" or loss.ignore_index != -100 or loss.label_smoothing != 0.0:
            raise ValueError("train_minibatch needs CrossEntropyLoss's default arguments")
        opt = self.optimizer
        if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
            raise ValueError("train_minibatch needs one torch.optim.Adam parameter group")
        g = opt.param_groups[0]
        if (tuple(g["betas"]) != (0.9, 0.999) or g["eps"] != 1e-8 or g["weight_decay"] != 0
                or g["amsgrad"] or g.get("maximize") or g.get("capturable") or g.get("differentiable")
                or g.get("fused") or isinstance(g["lr"], torch.Tensor)):
            raise ValueError("train_minibatch needs Adam's default hyperparameters (any lr)")
        seq = getattr(self.model, "layers", None)
        mods = list(seq.children()) if isinstance(seq, torch.nn.Sequential) else []
        linears = [m for m in mods if type(m) is torch.nn.Linear]
        chain = bool(linears) and len(mods) == 2 * len(linears) - 1 and all(
            type(m) is (torch.nn.ReLU if i % 2 else torch.nn.Linear) for i, m in enumerate(mods))
        if not chain or any(m.bias is None for m in linears) or any(
                a.out_features != b.in_features for a, b in zip(linears, linears[1:])):
            raise ValueError("train_minibatch needs a plain chain of Linear layers with ReLU between "
                             "them (not MLP-9)")
        if len(linears) > _lib.LMI_MAX_LAYERS:
            raise ValueError(f"more than {_lib.LMI_MAX_LAYERS} Linear layers")
        dims = [linears[0].in_features] + [m.out_features for m in linears]
        if max(dims) > _lib.LMI_TRAIN_MAX_DIM:
            raise ValueError(f"layer width {max(dims)} above LMI_TRAIN_MAX_DIM = {_lib.LMI_TRAIN_MAX_DIM}")
        params = [p for m in linears for p in (m.weight, m.bias)]
        if len(params) != len(g["params"]) or any(a is not b for a, b in zip(params, g["params"])):
            raise ValueError("the optimizer does not hold exactly the model's parameters")
        if any(p.dtype != torch.float32 for p in params):
            raise ValueError("train_minibatch trains float32 parameters")
        return linears

    def _minibatch_desc(self, linears):
        """(lmi_mlp_train_desc over the parameters and Adam's moments, steps
        taken so far); creates the optimizer state as Adam._init_group does."""
        from . import _lib
        opt = self.optimizer
        desc = _lib.MlpTrainDesc()
        desc.n_layers = len(linears)
        desc.dims[0] = linears[0].in_features
        t0 = None
        for i, m in enumerate(linears):
            desc.dims[i + 1] = m.out_features
            for p, names in ((m.weight, ("W", "W_exp_avg", "W_exp_avg_sq")),
                             (m.bias, ("b", "b_exp_avg", "b_exp_avg_sq"))):
                if not p.is_contiguous() or p.device.type != "cuda":
                    raise ValueError("parameters must be contiguous on the model's HIP device")
                st = opt.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not (st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
                    raise ValueError("Adam's moments must be contiguous")
                t = int(st["step"])
                if t0 is not None and t != t0:
                    raise ValueError("the parameters' Adam step counts differ")
                t0 = t
                for name, ten in zip(names, (p, st["exp_avg"], st["exp_avg_sq"])):
                    getattr(desc, name)[i] = ten.data_ptr()
        return desc, t0

    def train_minibatch(self, data_X, data_y, epochs=1, batch_size=256, generator=None, logger=None):
        """`epochs` passes over (data_X, data_y) with one Adam step per
        minibatch of `batch_size` rows -- what train_batch's loop would do if it
        stepped inside its inner loop (model.py:185-199) -- on the fused
        training kernels (lmi_mlp_train_steps; float32).  Each pass visits the
        rows in the order torch.randperm(n, generator=generator) (None: the
        global CPU generator, as SubsetRandomSampler draws it); its last
        minibatch is short when n % batch_size != 0.  Returns the per-epoch
        mean loss over the rows (each step's loss taken before its update).

        The weights are trained in place, and Adam's moments and step count
        live in self.optimizer.state in torch's own layout, so train /
        train_batch / another train_minibatch continue from them."""
        import ctypes as C
        from . import _lib
        linears = self._minibatch_linears()
        if int(batch_size) < 1 or int(epochs) < 0:
            raise ValueError("batch_size < 1 or epochs < 0")
        data_X = torch.as_tensor(data_X)
        data_y = torch.as_tensor(data_y)
        n_cls = linears[-1].out_features
        if data_X.dim() != 2 or data_X.shape[1] != linears[0].in_features or data_X.shape[0] < 1:
            raise ValueError("data_X must be (n >= 1, input_dim)")
        if data_y.shape != (data_X.shape[0],) or data_y.is_floating_point():
            raise ValueError("data_y must be n integer labels")
        if int(data_y.min()) < 0 or int(data_y.max()) >= n_cls:
            raise ValueError("a label lies outside [0, n_classes)")
        if self.device.type != "cuda":
            raise RuntimeError("train_minibatch runs on the GPU training kernels (no CPU fallback): "
                               "no HIP device")
        lib = _lib.load()
        opt, group = self.optimizer, self.optimizer.param_groups[0]
        n, batch = int(data_X.shape[0]), int(batch_size)
        steps = -(-n // batch)
        losses = []
        with torch.cuda.device(self.device), torch.no_grad():
            x = data_X.to(self.device, torch.float32).contiguous()
            y = data_y.to(self.device).to(torch.int32)
            desc, t0 = self._minibatch_desc(linears)
            need = lib.lmi_mlp_train_workspace_bytes(C.byref(desc), batch)
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            weights = torch.full((steps,), float(batch), dtype=torch.float64)
            weights[-1] = n - (steps - 1) * batch
            try:
                for ep in range(int(epochs)):
                    order = torch.randperm(n, generator=generator).to(self.device)
                    loss = torch.empty(steps, dtype=torch.float32, device=self.device)
                    _lib.check("lmi_mlp_train_steps", lib.lmi_mlp_train_steps(
                        C.byref(desc), x.data_ptr(), n, x.stride(0), y.data_ptr(), order.data_ptr(), n,
                        batch, 0, steps, t0, float(group["lr"]), 0.9, 0.999, 1e-8, loss.data_ptr(),
                        ws.data_ptr(), need, _lib.stream_handle(self.device)))
                    t0 += steps
                    losses.append(float((loss.cpu().double() * weights).sum() / n))  # waits for the epoch
                    if logger:
                        logger.info(f"Epoch {ep} | Loss {losses[-1]:.5f}")
            finally:
                for m in linears:
                    for p in (m.weight, m.bias):
                        opt.state[p]["step"] = torch.tensor(float(t0), dtype=torch.float32)
                # the kernels wrote the parameters behind torch's back
                # (p._version did not move): drop the cached device router
                self._router = None
                self._router_version = None
        return losses

    # ---- inference on the GPU --------------------------------------------------
    def router(self):
        """DeviceRouter over the current weights (rebuilt after training)."""
        from .index import DeviceRouter
        version = tuple(p._version for p in self.model.parameters())
        if self._router is None or self._router_version != version:
            self._router = DeviceRouter.from_module(self.model, device=self.device)
            self._router_version = version
        return self._router

    def predict(self, data_X: torch.FloatTensor):
        """argmax of the logits (model.py:201-212) -> int64 ndarray."""
        self.model.eval()
        out = self.router().argmax(data_X.to(self.device))
        return out.cpu().numpy().astype(np.int64)

    def predict_proba(self, data_X: torch.FloatTensor):
        """(probs, classes) over all classes, descending (model.py:214-229).

        A 1-D input raises IndexError as the reference does: it takes the
        softmax over dim 0 and then `prob.topk(prob.shape[1])` (model.py:222-227)
        indexes a shape of length 1."""
        self.model.eval()
        x = data_X.to(self.device)
        if x.dim() == 1:
            raise IndexError("tuple index out of range (predict_proba of a 1-D input, "
                             "reference model.py:227)")
        r = self.router()
        classes, probs = r.topr(x, r.n_classes, with_probs=True)
        return probs.cpu().numpy(), classes.cpu().numpy().astype(np.int64)


class LIDataset(torch.utils.data.Dataset):
    def __init__(self, dataset_x, dataset_y):
        self.dataset_x, self.dataset_y = data_to_torch(dataset_x, dataset_y)

    def __len__(self):
        return self.dataset_x.shape[0]

    def __getitem__(self, idx):
        return self.dataset_x[idx - 1], self.dataset_y[idx - 1]
