"""One rank of tests/test_gpu_essential_factors.py::test_view_graph_sharded_two_ways_over_gloo: the view graph (poses under
EssentialMatrixConstraint edges, free EssentialMatrix variables with priors and epipolar factors) on a sharded handle and on
a single one, as tests/_shard_worker.py does for the pose graphs."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from gtsam_petercdev_amd import _abi as A, _lib, distributed as D  # noqa: E402
from tests import _essential_restatement as S  # noqa: E402


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def main():
    rank, _, world = D.env_rank()
    dist = D.init("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    allreduce = D.torch_allreduce(dist, dev)
    calls = {"n": 0}

    def counted(ptr, count):
        calls["n"] += 1
        allreduce(ptr, count)

    arr = S.view_graph(n_poses=12, n_e=6)
    ref = _lib.ProductBackend(arr, device=0)
    sh = _lib.ProductBackend(arr, device=0)
    ordering = ref.compute_ordering(A.ORDER_ND)
    sh.set_shard(rank, world, counted)
    ref.set_ordering(ordering)
    sh.set_ordering(ordering)
    info, owner, owned = sh.shard_info()
    new = [f for f in range(arr.n_factors)
           if int(arr.f_type[f]) in (S.F_E, S.F_E_CONSTRAINT) or int(arr.var_types[arr.f_vars[arr.f_key_ptr[f]]]) == S.ESSENTIAL]
    r = {"info": info, "owners": sorted(set(owner.tolist())), "n_new": len(new), "owned_new": [f for f in new if owned[f]]}
    r["error0"] = [sh.error(), ref.error()]
    ref.linearize()
    sh.linearize()
    r["hdiag"] = relerr(sh.hessian_diagonal(), ref.hessian_diagonal())
    steps = []
    for lam, diag in ((0.0, False), (1e-3, False), (1.0, True)):
        ds, dr = sh.solve(lam, diag), ref.solve(lam, diag)
        es, er = sh.linear_error(), ref.linear_error()
        ts, tr_ = sh.retract(None, commit=False), ref.retract(None, commit=False)
        steps.append({"delta": relerr(ds, dr), "lin": [list(es), list(er)], "trial": [ts, tr_]})
    r["steps"] = steps
    params = A.lm_params_legacy()
    params.max_iterations = 8
    sh.set_values(arr.values)
    ref.set_values(arr.values)
    rs, rr = sh.lm_optimize(params), ref.lm_optimize(params)
    r["lm"] = {"accepted": [rs["trace_accepted"].tolist(), rr["trace_accepted"].tolist()],
               "final": [rs["final_error"], rr["final_error"]], "trace": relerr(rs["trace_error"], rr["trace_error"]),
               "values": relerr(sh.get_values(), ref.get_values())}
    sh.close()
    ref.close()
    gathered = [None] * world
    dist.all_gather_object(gathered, r)
    if rank == 0:
        print(json.dumps({"world": world, "ranks": gathered, "allreduce_calls": calls["n"]}))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
