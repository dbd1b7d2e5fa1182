"""Timing of the a posteriori indicator and the refinement at 1e6 elements on one MI355X (DESIGN.md
section 11): lssvr_estimate (M = 9, nq = 16, in-kernel sin rhs) and lssvr_refine (theta = 0.5), device
events around `reps` back-to-back launches after a warm-up, beside lssvr_enhance on the same mesh.
``--varcoef`` adds lssvr_estimate_varcoef (same M and nq; a, a', f tables) in both table layouts.
``--reaction`` (with ``--varcoef``) adds lssvr_estimate_react (a fourth table, c) and its ratio to the varcoef entry.
``--hp`` adds the three hp entries on the same W (ldw = M): lssvr_smoothness, lssvr_refine_hp (sigma_min = 1, dM = 2,
M_max = 21) and lssvr_group_by_degree (degrees 5 .. 21 mixed), each against its HBM bound.
Prints the algorithmic bytes and flops per element, the bound that applies and the fraction of it;
``--json PATH`` also writes the record as JSON.

    python scripts/adapt_quick.py [--ne 1000000] [--reps 50] [--varcoef [--reaction]] [--hp] [--json PATH]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hybrid_fem_lssvr_amd import ops  # noqa: E402

FP64_PEAK_TFLOPS = 78.6      # MI355X vector FP64 peak
HBM_PEAK_GBS = 8000.0        # spec; 6290 GB/s measured stream rate


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def roofline(name, t, ne, bytes_pe, flops_pe):
    tb = bytes_pe * ne / (HBM_PEAK_GBS * 1e9)
    tf = flops_pe * ne / (FP64_PEAK_TFLOPS * 1e12)
    bound = "hbm" if tb >= tf else "fp64"
    frac = max(tb, tf) / t
    print(f"{name}: {t * 1e6:8.1f} us  {bytes_pe:.0f} B/elem, {flops_pe:.0f} flop/elem "
          f"(intensity {flops_pe / bytes_pe:.1f} flop/B, ridge 9.8) -> {bound}-bound, "
          f"{frac * 100:.1f}% of the {bound} bound ({bytes_pe * ne / t / 1e9:.0f} GB/s, "
          f"{flops_pe * ne / t / 1e12:.2f} TFLOP/s)")
    return dict(us=t * 1e6, bytes_per_element=bytes_pe, flops_per_element=flops_pe, bound=bound, frac=frac)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--varcoef", action="store_true", help="also time lssvr_estimate_varcoef, both layouts")
    ap.add_argument("--reaction", action="store_true", help="with --varcoef: also time lssvr_estimate_react")
    ap.add_argument("--hp", action="store_true", help="also time lssvr_smoothness, lssvr_refine_hp, lssvr_group_by_degree")
    ap.add_argument("--json", default=None, help="write the record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adapt_quick.py needs an MI355X")
    dev = torch.device("cuda:0")
    ne, M, nq, ncol = args.ne, 9, 16, 12
    rng = np.random.default_rng(0)
    h = rng.uniform(0.5, 1.5, ne)
    x_h = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    x = torch.as_tensor(x_h, device=dev)
    u = torch.sin(np.pi * x)
    rhs = (ops.POISSON_AMP, ops.POISSON_OMEGA)
    gd = (float(x_h[0]), float(x_h[-1]))          # given: no device-to-host read per call
    W, _ = ops.enhance(x, u, M, 1e4, ncol, rhs=rhs, global_domain=gd)
    work = ops.adapt_work(x, ne)
    eta2, _, out3 = ops.estimate(x, W, nq, rhs=rhs, work=work)
    t_enh = timeit(lambda: ops.enhance(x, u, M, 1e4, ncol, rhs=rhs, global_domain=gd, out=W), args.reps)
    t_est = timeit(lambda: ops.estimate(x, W, nq, rhs=rhs, work=work), args.reps)
    # refine: the launches alone (no trimming synchronisation) through the C entry
    lib = ops._capi.load()
    x_new = torch.empty(2 * ne + 1, dtype=torch.float64, device=dev)
    ne_new = torch.empty(1, dtype=torch.int64, device=dev)
    st = ops._stream(None)

    def ref():
        ops._capi.check(lib.lssvr_refine(x.data_ptr(), ne, eta2.data_ptr(), out3[1:2].data_ptr(), 0.5, 0.0,
                                         work.data_ptr(), x_new.data_ptr(), None, ne_new.data_ptr(), st),
                        "lssvr_refine")
    t_ref = timeit(ref, args.reps)
    n_new = int(ne_new.item())
    # algorithmic traffic and work per element
    est_bytes = 8 * (M + 1) + 8                               # W row + x (shared nodes), eta2
    sin_flops = 2 * 10 + 10                                   # odd polynomial through r^21 + reduction
    est_flops = nq * (2 * (M - 2) + 1 + 2 + 2 + sin_flops + 2) + 4 * (M - 1) + 12
    ref_bytes = 2 * (8 + 8) + (n_new - ne) / ne * 8 + 8       # x, eta2 twice (count, scatter), x_new
    ref_flops = 6
    rec = {"ne": ne, "M": M, "nq": nq, "n_colloc_enhance": ncol, "reps": args.reps,
           "enhance_us": t_enh * 1e6, "marked": n_new - ne}
    print(f"ne = {ne}, M = {M}, nq = {nq}; lssvr_enhance (n_colloc = {ncol}) {t_enh * 1e6:.1f} us")
    rec["estimate"] = roofline("lssvr_estimate", t_est, ne, est_bytes, est_flops)
    rec["refine"] = roofline("lssvr_refine  ", t_ref, ne, ref_bytes, ref_flops)
    rec["estimate_over_enhance"] = t_est / t_enh
    rec["refine_over_enhance"] = t_ref / t_enh
    print(f"estimate / enhance = {t_est / t_enh:.3f}, refine / enhance = {t_ref / t_enh:.3f}, "
          f"marked {n_new - ne} of {ne}")
    if args.varcoef:
        # a = 1 + 0.5 sin(3x), a', f tabulated at the estimator's points; a_ends from a at the nodes
        xq = ops.estimate_points(x, nq)
        a_tab = 1.0 + 0.5 * torch.sin(3.0 * xq)
        tabs = [a_tab, 1.5 * torch.cos(3.0 * xq), ops.POISSON_AMP * torch.sin(ops.POISSON_OMEGA * xq)]
        an = 1.0 + 0.5 * torch.sin(3.0 * x)
        a_ends = torch.stack([an[:-1], an[1:]], dim=1).contiguous()
        # tables a, a', f + a_ends + W row + x (shared nodes) + eta2
        vc_bytes = 3 * nq * 8 + 16 + 8 * M + 8 + 8
        # per point: two M-1 term sums (u', u''), 4 for the residual, 2 for the weighted square; end fluxes
        vc_flops = nq * (4 * (M - 1) + 4 + 2) + 4 * (M - 1) + 2 + 14
        for pm in (True, False):
            tt = [t.t().contiguous() for t in tabs] if pm else tabs
            t_vc = timeit(lambda: ops.estimate_varcoef(x, W, nq, *tt, a_ends, point_major=pm, work=work), args.reps)
            key = "estimate_varcoef_" + ("point_major" if pm else "element_major")
            rec[key] = roofline("lssvr_estimate_varcoef (%s)" % ("point-major" if pm else "element-major"),
                                t_vc, ne, vc_bytes, vc_flops)
            if args.reaction:
                c_tab = 2.0 + torch.cos(2.0 * np.pi * xq)
                c_tab = c_tab.t().contiguous() if pm else c_tab
                t_rx = timeit(lambda: ops.estimate_varcoef(x, W, nq, *tt, a_ends, point_major=pm, work=work,
                                                           c_values=c_tab), args.reps)
                key = "estimate_react_" + ("point_major" if pm else "element_major")
                # one more table; per point one more M-term sum (u) and 2 for -c u
                rec[key] = roofline("lssvr_estimate_react   (%s)" % ("point-major" if pm else "element-major"),
                                    t_rx, ne, vc_bytes + nq * 8, vc_flops + nq * (2 * (M - 1) + 2))
                rec[key]["over_varcoef"] = t_rx / t_vc
                print(f"    estimate_react / estimate_varcoef = {t_rx / t_vc:.3f} (bytes {vc_bytes + nq * 8} / "
                      f"{vc_bytes} = {(vc_bytes + nq * 8) / vc_bytes:.3f})")
    if args.hp:
        deg = torch.full((ne,), M, dtype=torch.int32, device=dev)
        sigma = torch.empty(ne, dtype=torch.float64, device=dev)
        deg_new = torch.empty(2 * ne, dtype=torch.int32, device=dev)
        cnt = torch.empty(3, dtype=torch.int64, device=dev)

        def smooth():
            ops._capi.check(lib.lssvr_smoothness(W.data_ptr(), M, deg.data_ptr(), ne, sigma.data_ptr(), st),
                            "lssvr_smoothness")

        def ref_hp():
            ops._capi.check(lib.lssvr_refine_hp(x.data_ptr(), ne, eta2.data_ptr(), out3[1:2].data_ptr(), 0.5, 0.0,
                                                sigma.data_ptr(), deg.data_ptr(), 1.0, 2, 21, work.data_ptr(),
                                                x_new.data_ptr(), deg_new.data_ptr(), None, cnt[0:1].data_ptr(),
                                                cnt[1:3].data_ptr(), st), "lssvr_refine_hp")
        t_sm = timeit(smooth, args.reps)
        t_hp = timeit(ref_hp, args.reps)
        n_hp, n_split, n_raised = (int(v) for v in cnt.cpu())
        mixed = torch.as_tensor(rng.integers(5, 22, ne).astype(np.int32), device=dev)
        ids = torch.empty(ne, dtype=torch.int64, device=dev)
        offsets = torch.empty(35, dtype=torch.int64, device=dev)
        gwork = torch.empty(lib.lssvr_group_work_bytes(ne) // 8, dtype=torch.float64, device=dev)

        def group():
            ops._capi.check(lib.lssvr_group_by_degree(mixed.data_ptr(), ne, ids.data_ptr(), offsets.data_ptr(),
                                                      gwork.data_ptr(), st), "lssvr_group_by_degree")
        t_gr = timeit(group, args.reps)
        # W row, deg, sigma; one log (~40 flop) + ~10 flop per coefficient
        rec["smoothness"] = roofline("lssvr_smoothness     ", t_sm, ne, 8 * M + 4 + 8, 50 * (M - 1))
        # x, eta2, sigma, deg twice (count, scatter); x_new, deg_new of the new elements
        rec["refine_hp"] = roofline("lssvr_refine_hp      ", t_hp, ne, 2 * (8 + 8 + 8 + 4) + n_hp / ne * 12, 8)
        # deg twice (histogram, scatter), ids
        rec["group_by_degree"] = roofline("lssvr_group_by_degree", t_gr, ne, 2 * 4 + 8, 1)
        rec["refine_hp"].update(bisected=n_split, raised=n_raised)
        for k, t in (("smoothness", t_sm), ("refine_hp", t_hp), ("group_by_degree", t_gr)):
            rec[k]["over_estimate"] = t / t_est
        print(f"smoothness / estimate = {t_sm / t_est:.3f}, refine_hp / estimate = {t_hp / t_est:.3f}, "
              f"group_by_degree / estimate = {t_gr / t_est:.3f}, refine_hp / refine = {t_hp / t_ref:.3f}; "
              f"refine_hp bisected {n_split}, raised {n_raised} of {ne}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
