"""k-means for 128 < d <= 1024 on the GPU (kmeans_assign_wide_kernel,
csrc/lmi_kmeans.hip): a row no longer fits in registers, so the kernel tiles
the centroids instead -- and must still give the narrow kernel's arithmetic,
which oracle.kmeans_assign states for any d: bit for bit in labels and
distances.  Shapes: one point / one centroid; d % 4 != 0 (rows not 16-byte
aligned: the scalar-load variant) and d % 4 == 0; d that is no multiple of
the 32-column register block or the 128-column LDS chunk; k below, at no
multiple of, and above the 32-centroid tile; more than one workgroup; the
reference's own 768 x 122; the limit 1024."""
import numpy as np
import pytest
import torch

import lmi_oracle as O
from li import _lib
from li import kmeans as K

pytestmark = pytest.mark.gpu


def _blobs(n, d, c, seed, spread=0.15):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((c, d)).astype(np.float32)
    lab = rng.integers(0, c, n)
    return (centres[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n,d,k", [(1, 129, 1), (777, 130, 7), (3001, 200, 40), (513, 1000, 5),
                                   (2000, 768, 122), (1500, 1024, 300)])
def test_assign_wide_bitwise(n, d, k):
    x = _blobs(n, d, max(2, k // 3), n + d)
    cent = _blobs(k, d, max(2, k // 3), k)
    lab, dist = K.assign(torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda())
    ol, od = O.kmeans_assign(x, cent)
    assert (lab.cpu().numpy() == ol).all()
    assert (_bits(dist.cpu().numpy()) == _bits(od)).all()


def test_assign_wide_unaligned_base():
    """d % 4 == 0 but x itself starts 4 bytes off a 16-byte boundary (a view
    into a larger buffer): the scalar-load variant, same bits."""
    n, d, k = 300, 132, 9
    x = _blobs(n, d, 4, 1)
    cent = _blobs(k, d, 4, 2)
    buf = torch.zeros(n * d + 1, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda().ravel()
    xv = buf[1:].view(n, d)
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    lab, dist = K.assign(xv, torch.from_numpy(cent).cuda())
    ol, od = O.kmeans_assign(x, cent)
    assert (lab.cpu().numpy() == ol).all()
    assert (_bits(dist.cpu().numpy()) == _bits(od)).all()


def test_assign_wide_ties_and_duplicates():
    """test_gpu_kmeans.test_assign_ties_and_duplicates at d = 768: the strict
    minimum keeps the lowest centroid index, within a tile and across the
    column chunks."""
    x = np.zeros((300, 768), np.float32)
    x[::2, 3] = 1.0
    cent = np.zeros((6, 768), np.float32)
    cent[[1, 4], 3] = 1.0  # 0,2,3,5 tie at the origin; 1 and 4 tie at e_3
    lab, _ = K.assign(torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda())
    assert (lab.cpu().numpy() == np.where(np.arange(300) % 2 == 0, 1, 0)).all()
    # ties across two centroid tiles (k > 32): 40 identical centroids -> index 0
    lab, _ = K.assign(torch.from_numpy(x).cuda(), torch.zeros((40, 768), device="cuda"))
    assert (lab.cpu().numpy() == 0).all()


def test_wider_than_the_limit_raises():
    assert _lib.LMI_KMEANS_MAX_D == 1024
    x = torch.zeros((4, 1025), device="cuda")
    with pytest.raises(Exception, match="1024"):
        K.assign(x, torch.zeros((2, 1025), device="cuda"))
    with pytest.raises(ValueError):
        K.Kmeans(1025, 2)
    K.Kmeans(1024, 2)


@pytest.mark.parametrize("n,d,k", [(999, 200, 9), (40000, 768, 122)])
def test_update_wide_bitwise(n, d, k):
    x = _blobs(n, d, k, 11)
    rng = np.random.default_rng(2)
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[lab == k - 1] = 0  # one empty cluster keeps its row
    cent = rng.standard_normal((k, d)).astype(np.float32)
    c_dev = torch.from_numpy(cent).cuda()
    cnt = K.update(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), c_dev)
    oc, ocnt = O.kmeans_update(x, lab, cent)
    assert (cnt.cpu().numpy() == ocnt).all()
    assert (_bits(c_dev.cpu().numpy()) == _bits(oc)).all()


def test_train_wide_bitwise_with_oracle():
    n, d, k, mppc = 3000, 256, 16, 8
    x = _blobs(n, d, k, 5)
    km = K.Kmeans(d, k, niter=12, seed=2023, max_points_per_centroid=mppc)
    km.train(x)
    oc, oobj = O.kmeans_train(x, k, niter=12, seed=2023, max_points_per_centroid=mppc)
    assert (_bits(km.centroids) == _bits(oc)).all()
    np.testing.assert_allclose(km.obj, oobj, rtol=1e-9)
    D, I = km.index.search(x, 1)
    ol, od = O.kmeans_assign(x, oc)
    assert I.shape == (n, 1) and I.dtype == np.int64 and (I[:, 0] == ol).all()
    assert (_bits(D[:, 0]) == _bits(od)).all()
