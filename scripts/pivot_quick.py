"""A/B of the pivoting against the unpivoted tridiagonal solve on one GPU, in one run: event brackets around REPS
back-to-back calls of each C entry on preallocated buffers, the two solvers interleaved round by round, median and
spread over the rounds.  Both are measured the same way, so launch gaps between the small kernels of the coarse levels
are in both numbers.

    python scripts/pivot_quick.py [ne=1000000] [rounds=15]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hybrid_fem_lssvr_amd import _capi, ops  # noqa: E402

REPS = 50


def main():
    ne = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    dev = torch.device("cuda:0")
    lib = _capi.load()
    x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    bq = torch.full_like(xq, 0.5 * ne / 2.0)                       # cell Peclet 0.25: both solvers may run it
    b = ops.p1_assemble(x, 2, rhs=(ops.POISSON_AMP, ops.POISSON_OMEGA), c_quad=torch.ones_like(xq), b_quad=bq)
    st = torch.cuda.current_stream().cuda_stream
    kap = (_capi.C.c_double * 2)(0.0, 0.0)
    out = {}
    for nc in (1, 8):
        load = b["load"].repeat(nc, 1).contiguous()
        bc = torch.zeros((nc, 2), dtype=torch.float64, device=dev)
        u_a, u_b = torch.empty_like(load), torch.empty_like(load)
        wa = torch.empty(lib.lssvr_tridiag_multi_work_bytes(ne, nc), dtype=torch.uint8, device=dev)
        wb = torch.empty(lib.lssvr_tridiag_pivot_work_bytes(ne, nc), dtype=torch.uint8, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda t: t.data_ptr()                                              # noqa: E731

        def run_a():
            return lib.lssvr_tridiag_ns_dirichlet_solve_multi(p(b["diag"]), p(b["sub"]), p(b["sup"]), p(load), ne, nc,
                                                              p(bc), p(u_a), p(wa), wa.numel(), st)

        def run_b():
            return lib.lssvr_tridiag_pivot_solve_multi(p(b["diag"]), p(b["sub"]), p(b["sup"]), p(load), 0, 0, p(bc),
                                                       kap, ne, nc, p(u_b), p(info), p(wb), wb.numel(), st)

        times = {"unpivoted": [], "pivot": []}
        for fn in (run_a, run_b):
            for _ in range(10):
                assert fn() == 0
        torch.cuda.synchronize()
        for r in range(rounds):
            order = (("unpivoted", run_a), ("pivot", run_b)) if r % 2 == 0 else (("pivot", run_b), ("unpivoted", run_a))
            for name, fn in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / REPS)
        diff = float((u_a - u_b).abs().max().item())
        med = {k: statistics.median(v) for k, v in times.items()}
        out[nc] = med
        for k, v in times.items():
            print(f"ne={ne} nc={nc} {k}: median {med[k]:.1f} us (min {min(v):.1f}, max {max(v):.1f}, {rounds} rounds x "
                  f"{REPS} calls)")
        print(f"ne={ne} nc={nc} ratio pivot / unpivoted = {med['pivot'] / med['unpivoted']:.2f}, max |u difference| "
              f"{diff:.2e}, info {int(info.item())}")
    return out


def coarsest(rounds=15):
    """The coarsest level alone: a call with 32 unknowns (33 elements, two Dirichlet ends) is the end-value kernel and
    piv_base_kernel, nothing else; its event-bracketed time per call bounds the coarsest level's share of a large call
    from above (it includes both launches)."""
    dev = torch.device("cuda:0")
    lib = _capi.load()
    ne = 33
    x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
    b = ops.p1_assemble(x, 2, rhs=(ops.POISSON_AMP, ops.POISSON_OMEGA))
    st = torch.cuda.current_stream().cuda_stream
    kap = (_capi.C.c_double * 2)(0.0, 0.0)
    for nc in (1, 8):
        load = b["load"].repeat(nc, 1).contiguous()
        bc = torch.zeros((nc, 2), dtype=torch.float64, device=dev)
        u = torch.empty_like(load)
        wb = torch.empty(lib.lssvr_tridiag_pivot_work_bytes(ne, nc), dtype=torch.uint8, device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        p = lambda t: t.data_ptr()                                              # noqa: E731

        def run():
            return lib.lssvr_tridiag_pivot_solve_multi(p(b["diag"]), p(b["off"]), p(b["off"]), p(load), 0, 0, p(bc),
                                                       kap, ne, nc, p(u), p(info), p(wb), wb.numel(), st)
        for _ in range(10):
            assert run() == 0
        torch.cuda.synchronize()
        t = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / REPS)
        print(f"coarsest level alone (32 unknowns, end-value kernel + piv_base_kernel) nc={nc}: median "
              f"{statistics.median(t):.1f} us (min {min(t):.1f}, max {max(t):.1f})")


if __name__ == "__main__":
    main()
    coarsest()
