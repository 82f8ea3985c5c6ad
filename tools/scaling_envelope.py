"""Figures of the lagged scaling's envelope for the library HMMBW_LIB names (default: the tree's): every
case of tests/scaling_ref.py through the forward-only scorer (all cases of a model as one ragged set, and each case
alone in full waves) and one E-step pass per model, default (lagged) and safe scaling, against the oracle.

    python tools/scaling_envelope.py LABEL OUT.json           one library's block
    python tools/scaling_envelope.py --combine OUT.json BLOCK.json [BLOCK.json ...]

A block holds the counts, the cases whose default-scaling log P misses 1e-9 with their relative errors (inf: -inf or
NaN where the oracle is finite), the models whose statistics miss 1e-9 or hold a NaN, and the largest
default-vs-safe differences.  profiles/scaling/envelope.json is the combination of a block of the library before the
bound was tightened and one of this tree's."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KEYS = (("pi_num", "log_pi_num"), ("xi", "log_xi"), ("gamma_den_excl", "log_gden_excl"),
        ("gamma_den_all", "log_gden_all"), ("B_num", "log_bnum"))
TOL = 1e-9


def ll_err(x, ref):
    x, ref = np.asarray(x, float), np.asarray(ref, float)
    e = np.zeros(len(ref))
    f = np.isfinite(ref) & np.isfinite(x)
    e[f] = np.abs(x[f] - ref[f]) / np.abs(ref[f])
    e[(np.isneginf(x) != np.isneginf(ref)) | np.isnan(x)] = np.inf
    return e


def stat_err(g, h):
    """Largest relative difference over the entries above the 1e-300 absolute term; inf with a NaN."""
    worst = 0.0
    for key, _ in KEYS:
        x, y = np.asarray(g[key], float), np.asarray(h[key], float)
        if np.any(np.isnan(x)):
            return float("inf")
        f = np.abs(y) > 1e-300
        if f.any():
            worst = max(worst, float(np.max(np.abs(x[f] - y[f]) / np.abs(y[f]))))
    return worst


def num(v):
    return float(f"{v:.3e}") if np.isfinite(v) else "inf"


def block(label):
    import scaling_ref as S
    import test_gpu_scaling as T
    from oracle import oracle as O
    O.load()
    v1 = S.regimes(S.lagged_regime_v1)
    miss, safe_miss, stat_miss, nan_models = {}, [], {}, []
    d_ll = d_stat = 0.0
    by_regime = {}
    for name in T.MODEL_NAMES:
        m = S.MODELS[name]
        cases = S.cases_of(name)
        obs = [c.obs for c in cases]
        ref = T.oracle_score(O, m, obs)
        lag, safe = T.score(m, obs, False), T.score(m, obs, True)
        e_lag, e_safe = ll_err(lag, ref), ll_err(safe, ref)
        d_ll = max(d_ll, T.rel_diff(lag, safe))
        for i, c in enumerate(cases):
            full = [c.obs] * max(8, T.V.layout_u(m.N))
            rf = T.oracle_score(O, m, full)
            lf, sf = T.score(m, full, False), T.score(m, full, True)
            d_ll = max(d_ll, T.rel_diff(lf, sf))
            e = max(float(e_lag[i]), float(ll_err(lf, rf).max()))
            kind = v1[c.name].kind
            n_all, n_miss = by_regime.get(kind, (0, 0))
            by_regime[kind] = (n_all + 1, n_miss + (e > TOL))
            if e > TOL:
                miss[c.name] = {"regime_v1": kind, "ragged": num(float(e_lag[i])), "full": num(float(ll_err(lf, rf).max()))}
            if max(float(e_safe[i]), float(ll_err(sf, rf).max())) > TOL:
                safe_miss.append(c.name)
        g, ll = T.estep(m, obs)
        gs, _ = T.estep(m, obs, safe_scaling=True)
        s = T.oracle_estep(O, m, obs)
        with np.errstate(under="ignore"):
            so = {k: np.exp(getattr(s, lk)) for k, lk in KEYS}
        e_stat = max(stat_err(g, so), float(ll_err(ll, s.logP).max()))
        if not e_stat <= TOL:
            stat_miss[name] = num(e_stat)
        if any(np.any(np.isnan(g[k])) for k, _ in KEYS):
            nan_models.append(name)
        else:
            d_stat = max(d_stat, stat_err(g, gs))
    return {"library": label, "cases": len(S.CASES), "models": len(S.MODELS), "tolerance": TOL,
            "cases_by_v1_regime (all, default log P misses)": {k: list(v) for k, v in sorted(by_regime.items())},
            "default_log_p_misses": miss, "safe_log_p_misses": safe_miss,
            "estep_default_misses (statistics or log P, worst relative error)": stat_miss,
            "models_with_nan_statistics": nan_models,
            "largest_default_vs_safe_log_p": num(d_ll),
            "largest_default_vs_safe_statistic (models without NaN)": num(d_stat)}


def main():
    if sys.argv[1] == "--combine":
        out = {"what": __doc__.split("\n\n")[0].replace("\n", " "),
               "blocks": [json.load(open(p)) for p in sys.argv[3:]]}
        json.dump(out, open(sys.argv[2], "w"), indent=1)
        return
    b = block(sys.argv[1])
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
    json.dump(b, open(sys.argv[2], "w"), indent=1)
    print(json.dumps({k: v for k, v in b.items() if k != "default_log_p_misses"}, indent=1))
    print("default log P misses:", len(b["default_log_p_misses"]))


if __name__ == "__main__":
    main()
