"""Makes tests/golden/truth_orders.npz: for a few pixels of the 64 x 48 Kerr frame of tests/test_orders.py that reach order 1 or order 2,
the observer's ray state, the end state of that order by DOP853 chained through the scene and the inflated-disk scene (tests/truth.py,
max_step 0.05), the CPU oracle's end state chained the same way, and for one order-1 pixel a polarization vector carried along the
whole geodesic by tests/polarization_truth.py.  CPU only, a few minutes:  python tests/golden/make_orders_truth.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import polarization_truth as PT   # noqa: E402
import test_orders as TO          # noqa: E402


def spread(idx, rho, count):
    """`count` entries of idx, evenly spaced in the order of rho (both ends included)"""
    order = np.argsort(rho)
    return idx[order[np.round(np.linspace(0, len(order) - 1, count)).astype(int)]]


def main():
    metric, objs = TO.kerr_scene()
    opt = TO.solver()
    s0, (leg0, orders) = TO.oracle_kerr_chain()
    picks = []
    for k, count in ((1, 4), (2, 2)):
        o = orders[k - 1]
        on = o["cont"]["hit"] == TO.DISK_OBJECT
        idx, se = o["idx"][on], o["cont"]["state_end"][on]
        for p in spread(idx, np.hypot(se[:, 1], se[:, 2]), count):
            picks.append((int(p), k, se[list(idx).index(p)]))
    rows = dict(pixel=[], order=[], s0=[], truth_end=[], oracle_end=[], lam=[])
    for p, k, oracle_end in picks:
        _, chain = TO.chain(TO.truth_leg(metric, opt), s0[p:p + 1], objs, k)
        assert len(chain) == k and all(c["cont"] is not None and c["cont"]["hit"][0] == TO.DISK_OBJECT for c in chain), (p, k)
        end = chain[-1]["cont"]["state_end"][0]
        lam = sum(float(c["cross"]["lambda_end"][0]) + float(c["cont"]["lambda_end"][0]) for c in chain)
        leg0_t = TO.truth_leg(metric, opt)(objs, s0[p:p + 1])
        lam += float(leg0_t["lambda_end"][0])
        print(f"pixel {p} order {k}: rho {np.hypot(end[1], end[2]):.3f}  |oracle - truth| {np.abs(oracle_end - end).max():.2e}  lambda {lam:.3f}", flush=True)
        for key, v in zip(("pixel", "order", "s0", "truth_end", "oracle_end", "lam"), (p, k, s0[p], end, oracle_end, lam)):
            rows[key].append(v)
    out = {k: np.array(v) for k, v in rows.items()}
    # one order-1 pixel: f_0 orthogonal to k_0, carried to the order-1 end along the one geodesic the chain follows
    q = 0
    x0, k0 = out["s0"][q][:4], out["s0"][q][4:]
    g0 = PT.g_at("ks_true", x0, 1.0, 0.9)
    f0 = PT.normalise(g0, np.array([0.0, 0.3, 1.0, 0.2]))
    e_t = np.array([1.0, 0, 0, 0])
    f0 = f0 - PT.inner(g0, f0, k0) / PT.inner(g0, e_t, k0) * e_t
    y, rmin = PT.transport("ks_true", 1.0, 0.9, x0, k0, f0, out["lam"][q], max_step=0.05)
    print("transported end against the chained end:", np.abs(y[:8] - out["truth_end"][q]).max(), "r_min", rmin,
          "kappa drift", np.abs(PT.kappa(y[:4], y[4:8], y[8:], 0.9) - PT.kappa(x0, k0, f0, 0.9)).max())
    assert np.abs(y[:8] - out["truth_end"][q]).max() <= 1e-9
    out.update(wp_row=np.array(q), wp_f0=f0, wp_f1=y[8:])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "truth_orders.npz"), **out)


if __name__ == "__main__":
    main()
