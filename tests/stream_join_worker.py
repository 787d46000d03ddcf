"""One process of tests/test_gpu_stream_join.py: a ONE-RANK RCCL process group
with LMI_FORCE_EXCHANGE=1 (as tests/rccl_worker.py), so the batch stream takes
its G > 1 branch -- F1, the captured all-gather, F2 -- with the scan in two
launches (join_cus): the late join goes onto the finish stream behind F2.
Eight launches over six batches, each answer compared bit for bit with a
Searcher that does not exchange, in both arithmetics.  Exits 0 and prints the
check when every comparison holds."""
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
    w = workloads.clustered(n=20_000, nq=300, C=8, seed=97, label_mode="skewed")
    ix = DeviceIndex(w["x"], w["labels"], w["C"], chunk_rows=256, device="cuda:0")
    router = DeviceRouter(w["layers"], device="cuda:0")
    sx = Searcher(ix, router)                    # exchange: forced
    s0 = Searcher(ix, router, exchange=False)    # the plain one-GPU path
    assert sx.exchange and not s0.exchange
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    eq = np.testing.assert_array_equal
    bs = []
    for i in range(6):
        p = np.random.default_rng(300 + i).permutation(w["q"].shape[0])
        bs.append((w["qn"][p], w["q"][p]))
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for dd in ("f32", "f64"):
        ref = [s0.search(T(a), T(b), 3, k=10, dist=dd) for a, b in bs]
        ss = sx.streamed(*bs[0], 3, k=10, dist=dd, join_cus=ncu // 4)
        assert ss.X and ss.join_cus == ncu // 4 and all((n, 0) in ss.graphs for n in ("SJ", "F1", "FX", "F2"))
        staged = []
        for t in range(8):
            ss.stage(*bs[t % 6])
            staged.append(t % 6)
            d, a = ss.step()
            i = staged[t - 3] if t >= 3 else 0
            eq(d, ref[i][0])
            eq(a, ref[i][1])
        ss.close()
    dist.barrier()
    dist.destroy_process_group()
    print("stream join under forced exchange OK")


if __name__ == "__main__":
    main()
