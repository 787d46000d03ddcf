"""lmi_router_stop (csrc/lmi_router.hip): the probability-mass stop rule fused
into K1's selection, on every dispatch of the router.

Which code each case reaches (tests/router_cases.py, tests/test_gpu_router.py):
  MLP-5, c3, nav768: router_mfma_kernel<1> -- its four-lane top-8 lists for
      R <= 8, select_classes' rank loop and second pass for R > 8
  odd, c65, one: router_kernel<32> -- select_classes' wave-wide rounds for
      R <= 8, the rank loop and second pass for R > 8 (c65)
  many-classes: router_kernel<16>
  mis768: misaligned weights, router_kernel<16> with scalar staging
N = 257 rows leave a partial tile in every kernel; every R of case.Rs() covers
both sides of the R <= 8 split and R = C.

The stop mass of a (case, R) is the median over the rows of S_h, h = ceil(R/2),
computed from the plain call's own probabilities: N is odd, so the median is
one row's S_h, that row and the rows above it drop probe h (strict <) and the
rows below keep it.  The rule is checked exactly: the kernel's mask against
li.index.probe_stop_mask on the kernel's own probabilities.  "Not degenerate"
is asserted as: some row has a dropped probe, and probe h is kept by some rows
and dropped by others (with a near-uniform router no row keeps all R probes at
such a stop mass, so "a row that kept everything" cannot be asked for)."""
import numpy as np
import pytest
import torch

import router_cases as RC
from li import _lib
from li.index import DeviceRouter, probe_stop_mask

pytestmark = pytest.mark.gpu

CASES = ["MLP-5", "c3", "nav768", "odd", "c65", "one", "many-classes", "mis768"]
N = 257


def _router(c):
    if c.name != "mis768":
        return DeviceRouter(c.layers), None
    # weight matrices at a 4-byte offset into a flat buffer (tests/test_gpu_router.py)
    layers, keep = [], []
    for w, b in c.layers:
        flat = torch.zeros(w.size + 1, device="cuda")
        flat[1:] = torch.from_numpy(w.reshape(-1)).cuda()
        keep.append(flat)
        layers.append((flat[1:].view(w.shape), torch.from_numpy(b).cuda()))
    r = DeviceRouter(layers)
    assert all(w.data_ptr() % 16 == 4 for w in r.W)
    return r, keep


def _mass_before(p, h):
    """S_h of every row: the float32 sum of p[:, :h] in ascending r."""
    s = np.zeros(p.shape[0], np.float32)
    for r in range(h):
        s = (s + p[:, r]).astype(np.float32)
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_router_stop(name):
    c = RC.case(name)
    assert c.n == N
    router, _keep = _router(c)
    x = torch.from_numpy(np.array(c.x)).cuda()
    for R in c.Rs():
        cls0, p0 = router.topr(x, R, with_probs=True)
        cls0, p0 = cls0.cpu().numpy(), p0.cpu().numpy()
        h = -(-R // 2)
        stop = min(1.0, float(np.median(_mass_before(p0, h))))
        for mp in (1, 2):
            nk = torch.full((N,), -7, dtype=torch.int32, device="cuda")
            cls, p = router.topr(x, R, with_probs=True, stop_mass=stop, min_probes=mp,
                                 n_probes_out=nk)
            cls, p, nk = cls.cpu().numpy(), p.cpu().numpy(), nk.cpu().numpy()
            # the probabilities of every pick, kept or not, are the plain call's
            assert np.array_equal(_bits(p), _bits(p0)), (name, R, mp)
            keep = probe_stop_mask(p, stop, mp)
            hist = np.bincount(keep.sum(1))
            print(f"{name} R={R} stop={stop:.6g} min={mp}: probes kept -> rows "
                  f"{ {int(i): int(hist[i]) for i in np.nonzero(hist)[0]} }")
            assert np.array_equal(cls >= 0, keep), (name, R, mp)
            assert np.array_equal(cls[keep], cls0[keep]), (name, R, mp)
            assert (cls[~keep] == _lib.LMI_PROBE_NONE).all(), (name, R, mp)
            assert np.array_equal(nk, keep.sum(1)), (name, R, mp)
            # a prefix, never shorter than min(mp, R)
            assert (np.diff(keep.astype(np.int8), axis=1) <= 0).all()
            assert (keep.sum(1) >= min(mp, R)).all()
            if R >= 2 and c.C >= 2 and mp <= h:
                assert (~keep).any(axis=1).any(), (name, R, mp, "no row was cut")
                assert keep[:, h].any() and not keep[:, h].all(), (name, R, mp, "degenerate mask")
            # without the probabilities and the counts: the same classes
            cls_b, none = router.topr(x, R, stop_mass=stop, min_probes=mp)
            assert none is None and np.array_equal(cls_b.cpu().numpy(), cls), (name, R, mp)
            # the out= form (a slice of a larger buffer, as the captured steps use it)
            buf = torch.full((N * R + 11,), -9, dtype=torch.int32, device="cuda")
            got, _ = router.topr(x, R, out=buf[5:5 + N * R], stop_mass=stop, min_probes=mp)
            assert got.data_ptr() == buf[5:].data_ptr()
            b = buf.cpu().numpy()
            assert np.array_equal(b[5:5 + N * R].reshape(N, R), cls), (name, R, mp)
            assert (b[:5] == -9).all() and (b[5 + N * R:] == -9).all()
        # every probe kept: the plain call
        nk = torch.empty((N,), dtype=torch.int32, device="cuda")
        cls, p = router.topr(x, R, with_probs=True, stop_mass=1.0, min_probes=R, n_probes_out=nk)
        assert np.array_equal(cls.cpu().numpy(), cls0) and np.array_equal(_bits(p.cpu().numpy()), _bits(p0))
        assert (nk.cpu().numpy() == R).all()
        # min_probes above R means R
        cls, _ = router.topr(x, R, stop_mass=stop, min_probes=R + 5)
        assert np.array_equal(cls.cpu().numpy(), cls0)


def test_plain_call_unchanged_by_the_rule_arguments():
    """stop_mass=None is lmi_router itself; n_probes_out then has no meaning."""
    c = RC.case("MLP-5")
    router = DeviceRouter(c.layers)
    x = torch.from_numpy(np.array(c.x)).cuda()
    a, pa = router.topr(x, 4, with_probs=True)
    b, pb = router.topr(x, 4, with_probs=True, stop_mass=None, min_probes=3)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    with pytest.raises(ValueError):
        router.topr(x, 4, n_probes_out=torch.empty(N, dtype=torch.int32, device="cuda"))
