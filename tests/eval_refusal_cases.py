"""The refusal order of the 13 evaluation entry points, by peeling: start from a call in which every argument that has a check is faulty at once,
record (code, message), repair the one argument whose repair changes the message, repeat until one repair is left (the call after it would be
accepted, so it is never made).  `extras` are single faults on an otherwise legal call: the other faulty values of an argument, and the checks that
need a second argument to be set.  Without a handle (the CPU half) the peeling stops at "null handle"; with one (the GPU half) the handle is an
argument like the others: NULL, then a ref_compat handle, then the live one.

tests/golden/eval_refusals.json holds what the parent commit's library answered (python -m tests.eval_refusal_cases OUT.json, with DESIRE_HIP_LIB
naming that library; the "gpu" half is recorded where a device is, the "cpu" half anywhere).  No kernel of these ops runs: every call is refused."""
import ctypes as C
import json
import os
import sys

SHAPE = (1, 4, 3, 6)                       # (n_scenes, mno, K, T_pred) of the live handle
K, T = SHAPE[2], SHAPE[3]
HZ = (2, 6)
NAN, INF = float("nan"), float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_refusals.json")

# pointer tokens: "Z" float input, "I" int32 input (zeros: a legal order), "P" uint8 input; ("O", name) an output buffer that must stay untouched
Z, I, P = "Z", "I", "P"


def O(name):
    return ("O", name)


def bad(faulty, good):                     # an argument with a check: faulty first
    return [faulty, good]


_UNITS = [("unit_x", bad(0.0, 1.0)), ("unit_y", bad(NAN, 1.0))]
_UNIT_EXTRAS = [dict(unit_x=v) for v in (-1.0, NAN, INF)] + [dict(unit_y=v) for v in (0.0, -2.0, INF)]
_RADIUS_EXTRAS = [dict(radius=v) for v in (NAN, INF)]
_HZ_EXTRAS = [dict(n_h=9), dict(n_h=-1), dict(host_horizons=(0, 6)), dict(host_horizons=(2, T + 1)), dict(host_horizons=(3, 3)), dict(host_horizons=(4, 2))]
_HZ = [("host_horizons", bad(None, HZ)), ("n_h", bad(0, 2))]


def _fit(order_name, lead):
    return dict(
        args=[("h", None)] + lead + [
            ("dev_fut", [Z]), ("n_modes", bad(0, 2)), ("t_end", bad(0, T)), ("iters", bad(-1, 2))] + _UNITS + [("var_floor", bad(-1.0, 1e-4))] + _HZ + [
            ("log_floor", bad(INF, -20.0)), ("dev_label", [O("label")]), ("dev_count", bad(None, O("count"))), ("dev_prob", bad(None, O("prob"))),
            ("dev_mean", [O("mean")]), ("dev_cov", [O("cov")]), ("dev_passes", [O("passes")]), ("dev_out", bad(None, O("out"))), ("dev_frame", [O("frame")])],
        extras=[dict(n_modes=K + 1), dict(n_modes=17), dict(t_end=T + 1), dict(iters=33), dict(var_floor=NAN), dict(log_floor=NAN),
                dict(dev_fut=None), dict(dev_fut=None, dev_out=None), dict(dev_fut=None, dev_out=None, dev_frame=None, **{order_name: None})] + _UNIT_EXTRAS + _HZ_EXTRAS)


def _plan(cond):
    tail = [("sigma", bad(0.0, 1.0)), ("t_cond", bad(0, 3))] if cond else []
    outs = [("dev_first", [O("first")]), ("dev_clear", [O("clear")]), ("dev_risk", bad(None, O("risk"))), ("dev_blame", [O("blame")])]
    if cond:
        outs += [("dev_cw", bad(None, O("cw"))), ("dev_dist", [O("dist")]), ("dev_ess", [O("ess")]), ("dev_support", [O("support")]), ("dev_cond", [O("cond")])]
    extras = [dict(dev_present=P), dict(M=-3)] + _RADIUS_EXTRAS + _UNIT_EXTRAS + _HZ_EXTRAS
    if cond:
        extras += [dict(t_cond=T + 1), dict(sigma=-1.0), dict(sigma=NAN), dict(sigma=INF)]
    return dict(args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_fut", bad(None, Z)), ("dev_present", [None]), ("dev_score", [Z]), ("dev_plans", bad(None, Z)),
                      ("dev_ego", [None]), ("M", bad(0, 2))] + _HZ + [("radius", bad(-1.0, 1.0))] + _UNITS + tail + outs,
                extras=extras)


def _recon(scene):
    outs = [("dev_e", [O("e")])] + ([("dev_E", [O("E")]), ("dev_count", [O("count")])] if scene else []) + [
        ("dev_w", [O("w")]), ("dev_winner", [O("winner")]), ("dev_recon", [O("recon")])]
    # ({}: the legal call on a handle without weights is refused by state, after every check of the arguments)
    return dict(args=[("h", None), ("dev_fut", bad(None, Z)), ("dev_Yhat", bad(None, Z)), ("mode", bad(3, 2)), ("tau", bad(NAN, 1.0))] + outs,
                extras=[dict(mode=-1), dict(tau=0.0), dict(tau=INF), dict(tau=-1.0), {}])


# per entry point: its arguments in the order of include/desire_hip.h, each with its values from the faultiest to the legal one, and the extras
OPS = {
    "desire_rank_samples": dict(
        args=[("h", None), ("dev_score", bad(None, Z)), ("dev_Yhat", bad(None, Z)), ("n_top", bad(0, 1)), ("dev_order", bad(None, O("order"))),
              ("dev_top_Y", [O("top_Y")]), ("dev_top_score", [O("top_score")])],
        extras=[dict(n_top=K + 1), dict(n_top=-1)]),
    "desire_ranked_errors": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_fut", bad(None, Z)), ("dev_order", bad(None, I)), ("n_top", bad(0, 1))] + _HZ + [
            ("unit_x", [1.0]), ("unit_y", [1.0]), ("dev_out", bad(None, O("out")))],
        extras=[dict(n_top=K + 1)] + _HZ_EXTRAS),
    "desire_kde_nll": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_fut", bad(None, Z)), ("dev_score", [Z])] + _HZ + _UNITS + [
            ("log_floor", bad(INF, -20.0)), ("dev_out", bad(None, O("out"))), ("dev_frame", [O("frame")])],
        extras=[dict(log_floor=NAN), dict(log_floor=-INF)] + _UNIT_EXTRAS + _HZ_EXTRAS),
    "desire_select_diverse": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_order", bad(None, I)), ("dev_score", bad(None, Z)), ("metric", bad(3, 0)), ("t_end", bad(0, T)),
              ("radius", bad(-1.0, 1.0))] + _UNITS + [("n_top", bad(0, 1)), ("dev_order_out", bad(None, O("order_out"))), ("dev_count", bad(None, O("count"))),
              ("dev_mass", [O("mass")]), ("dev_top_Y", [O("top_Y")]), ("dev_top_score", [O("top_score")])],
        extras=[dict(metric=-1), dict(t_end=T + 1), dict(t_end=-5), dict(n_top=K + 1)] + _RADIUS_EXTRAS + _UNIT_EXTRAS),
    "desire_joint_metrics": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_fut", bad(None, Z)), ("dev_present", [None]), ("dev_score", [Z])] + _HZ + [
            ("n_top", bad(0, 1)), ("radius", bad(-1.0, 1.0))] + _UNITS + [("dev_first", [O("first")]), ("dev_cnt", bad(None, O("cnt"))), ("dev_jerr", [O("jerr")]),
            ("dev_jscore", [O("jscore")]), ("dev_jorder", bad(None, O("jorder"))), ("dev_out", [O("out")])],
        extras=[dict(dev_present=P), dict(dev_fut=None, dev_present=P), dict(dev_fut=None, dev_present=P, dev_jerr=None), dict(n_top=K + 1)]
               + _RADIUS_EXTRAS + _UNIT_EXTRAS + _HZ_EXTRAS),
    "desire_select_worlds": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_present", [P]), ("dev_wscore", [Z]), ("metric", bad(3, 0)), ("reduce", bad(2, 0)), ("t_end", bad(0, T)),
              ("radius", bad(-1.0, 1.0))] + _UNITS + [("dev_worder", bad(None, O("worder"))), ("dev_wcount", bad(None, O("wcount"))), ("dev_wmass", [O("wmass")]),
              ("dev_wlabel", [O("wlabel")])],
        extras=[dict(metric=-1), dict(reduce=-1), dict(t_end=T + 1)] + _RADIUS_EXTRAS + _UNIT_EXTRAS),
    "desire_plan_risk": _plan(False),
    "desire_plan_risk_cond": _plan(True),
    "desire_fit_modes": _fit("dev_order", [("dev_Yhat", bad(None, Z)), ("dev_order", bad(None, I)), ("dev_score", [Z])]),
    "desire_fit_scene_modes": _fit("dev_worder", [("dev_Yhat", bad(None, Z)), ("dev_present", [P]), ("dev_worder", bad(None, I)), ("dev_wscore", [Z])]),
    "desire_occupancy": dict(
        args=[("h", None), ("dev_Yhat", bad(None, Z)), ("dev_fut", bad(None, Z)), ("dev_present", [None]), ("dev_score", [Z])] + _HZ + [
            ("mode", bad(2, 0)), ("Oh", bad(0, 4)), ("Ow", bad(0, 4)), ("dev_mask", bad(None, P)), ("dev_mask_of_scene", [I]), ("dev_occ", bad(None, O("occ"))),
            ("dev_exp", [O("exp")]), ("dev_hit", [O("hit")]), ("dev_viol", [O("viol")]), ("dev_off", [O("off")])],
        extras=[dict(dev_present=P), dict(dev_fut=None, dev_present=P), dict(mode=1), dict(mode=-1), dict(dev_mask_of_scene=None), dict(Oh=1025), dict(Ow=1025)]
               + _HZ_EXTRAS),
    "desire_recon_weights": _recon(False),
    "desire_recon_weights_scene": _recon(True),
}

_FLOATS = {"radius", "unit_x", "unit_y", "sigma", "var_floor", "log_floor", "tau"}


class Buffers:
    """What the pointer tokens stand for.  cpu: host arrays (never read: every call is refused); torch: device tensors, the outputs filled."""
    FILL = -7.0
    N = 4096

    def __init__(self, torch=None):
        self.torch, self.outs, self.keep = torch, {}, []
        if torch is None:
            host = (C.c_float * 64)()
            self.keep.append(host)
            self.ins = {Z: C.addressof(host), I: C.addressof(host), P: C.addressof(host)}
        else:
            z = torch.rand(self.N, device="cuda") + 0.5
            i = torch.zeros(self.N, device="cuda", dtype=torch.int32)
            p = torch.ones(self.N, device="cuda", dtype=torch.uint8)
            self.keep += [z, i, p]
            self.ins = {Z: z.data_ptr(), I: i.data_ptr(), P: p.data_ptr()}

    def ptr(self, tok):
        if tok is None:
            return None
        if tok in self.ins:
            return self.ins[tok]
        name = tok[1]
        if name not in self.outs:
            if self.torch is None:
                self.outs[name] = (C.c_float * 64)()
            else:
                self.outs[name] = self.torch.full((self.N,), self.FILL, device="cuda")
        o = self.outs[name]
        return C.addressof(o) if self.torch is None else o.data_ptr()

    def untouched(self):
        if self.torch is None:
            return all(not any(o) for o in self.outs.values())
        self.torch.cuda.synchronize()
        return all(bool((o == self.FILL).all()) for o in self.outs.values())


def _call(lib, fn, names, values, bufs):
    argv = []
    for n in names:
        v = values[n]
        if n == "h":
            argv.append(v)
        elif n == "host_horizons":
            argv.append(None if v is None else (C.c_int32 * 8)(*v))
        elif n in _FLOATS:
            argv.append(C.c_float(v))
        elif n.startswith("dev_"):
            argv.append(bufs.ptr(v))
        else:
            argv.append(int(v))
    rc = getattr(lib, fn)(*argv, None)
    if rc == 0:
        raise AssertionError("%s accepted a call that the cases hold to be faulty: %r" % (fn, {k: v for k, v in values.items() if k != "h"}))
    return [int(rc), lib.desire_last_error().decode()]


def peel(lib, fn, bufs, handles):
    """handles: the values of `h` from NULL to the live one ([None] without a device).  Returns {"peel": [[code, message, repaired], ...], "extras": ...}."""
    spec = OPS[fn]
    stages = {n: (list(handles) if n == "h" else list(v)) for n, v in spec["args"]}
    names = [n for n, _ in spec["args"]]
    at = {n: 0 for n in names}
    left = lambda: sum(len(stages[n]) - 1 - at[n] for n in names)
    cur = lambda: {n: stages[n][at[n]] for n in names}
    live = len(handles) > 1
    steps = []
    while True:
        got = _call(lib, fn, names, cur(), bufs)
        if left() <= (1 if live else 0):
            steps.append(got + [None])
            break
        repaired = None
        for n in names:
            if at[n] + 1 < len(stages[n]):
                at[n] += 1
                if _call(lib, fn, names, cur(), bufs) != got:
                    repaired = n
                    break
                at[n] -= 1
        steps.append(got + [repaired])
        if repaired is None:
            if live:
                raise AssertionError("%s: no single repair changes %r" % (fn, got))
            break
    good = {n: stages[n][-1] for n in names}
    extras = []
    for kw in spec["extras"]:
        extras.append([{k: (repr(v) if isinstance(v, float) else v) for k, v in kw.items()}] + _call(lib, fn, names, dict(good, **kw), bufs))
    return {"peel": steps, "extras": extras}


def run(lib, bufs, handles):
    return {fn: peel(lib, fn, bufs, handles) for fn in OPS}


def compare(got, want):
    """Every entry point and step that differs, by name: [] when the sequences are the recorded ones."""
    got = json.loads(json.dumps(got))
    diff = []
    for fn in sorted(set(got) | set(want)):
        for part in ("peel", "extras"):
            g, w = got.get(fn, {}).get(part, []), want.get(fn, {}).get(part, [])
            for i in range(max(len(g), len(w))):
                a, b = (g[i] if i < len(g) else None), (w[i] if i < len(w) else None)
                if a != b:
                    diff.append("%s %s[%d]: got %r, recorded %r" % (fn, part, i, a, b))
    return diff


def live_handles(_lib):
    """The live handle of SHAPE without weights, and the ref_compat handle of tests/test_gpu_plan.py's refusal test."""
    from tests.helpers import small_dims
    n, m, k, t = SHAPE
    h = _lib.Handle(small_dims(n_scenes=n, mno=m, K=k, T_obs=4, T_pred=t, n_grids=1, H=64))
    rc = _lib.Handle(small_dims(n_scenes=1, mno=4, K=1, T_obs=8, T_pred=8, H=16, n_grids=1, bn_mode=1, ref_compat=1, n_dec=2, posterior=1))
    return h, rc


def main(out_path, parent):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from desire_amd import _lib
    lib = _lib.load()
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["recorded_from"] = parent
    doc["shape"] = list(SHAPE)
    bufs = Buffers()
    doc["cpu"] = run(lib, bufs, [None])
    assert bufs.untouched()
    import torch
    if torch.cuda.is_available():
        bufs = Buffers(torch)
        h, rc = live_handles(_lib)
        doc["gpu"] = run(lib, bufs, [None, rc._h, h._h])
        assert bufs.untouched()
        h.close(); rc.close()
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded:", ", ".join("%s %d ops" % (k, len(doc[k])) for k in ("cpu", "gpu") if k in doc))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
