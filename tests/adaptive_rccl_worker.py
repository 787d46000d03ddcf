"""One process of tests/test_gpu_adaptive.py: a ONE-RANK RCCL process group
with LMI_FORCE_EXCHANGE=1 (as tests/rccl_worker.py), so the router's stop rule
runs on the exchange branch -- route_sharded in Searcher.search, the classes
routed into the gathered block in the batch stream -- and each answer is
compared bit for bit with a Searcher that does not exchange.  Exits 0 and
prints the checks when every comparison holds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "sisap23-laion-challenge-learned-index_amd"),
                os.path.join(ROOT, "oracle"), HERE]


def main():
    import numpy as np
    import torch
    import torch.distributed as dist

    import workloads
    from li.dist import init_from_env
    from li.index import DeviceIndex, DeviceRouter, Searcher
    os.environ["LMI_FORCE_EXCHANGE"] = "1"
    rank, world, _ = init_from_env()
    assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
    w = workloads.clustered(n=6000, d=768, nq=200, C=16, arch="MLP", label_mode="skewed")
    layers = [(a.copy(), b.copy()) for a, b in w["layers"]]
    layers[-1] = (layers[-1][0] * np.float32(100), layers[-1][1] * np.float32(100))
    ix = DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=512, device="cuda:0")
    router = DeviceRouter(layers, device="cuda:0")
    sx = Searcher(ix, router)                    # exchange: forced
    s0 = Searcher(ix, router, exchange=False)    # the plain one-GPU path
    assert sx.exchange and not s0.exchange
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    qn, q = T(w["qn"]), T(w["q"])
    eq = np.testing.assert_array_equal
    rule = dict(stop_mass=0.8, min_probes=1)
    cx, c0 = sx.route(qn, 4, **rule).cpu().numpy(), s0.route(qn, 4, **rule).cpu().numpy()
    eq(cx, c0)
    counts = np.bincount((c0 >= 0).sum(1), minlength=5)[1:]
    assert (counts > 0).all(), counts
    r0 = s0.search(qn, q, 4, k=10, **rule)
    eq(sx.search(qn, q, 4, k=10, **rule), r0)
    assert not np.array_equal(r0[1], s0.search(qn, q, 4, k=10)[1])
    ss = sx.streamed(w["qn"], w["q"], 4, k=10, **rule)
    assert ss.X
    for _ in range(3):
        eq(ss.step(), r0)
    ss.close()
    dist.barrier()
    dist.destroy_process_group()
    print(f"adaptive forced exchange OK: probe counts {counts.tolist()}")


if __name__ == "__main__":
    main()
