#!/usr/bin/env python3
"""Accuracy of fs_ppo_grad's two precisions (measurement only): per gradient tensor, the largest
|kernel - reference| / max|reference| and the largest elementwise relative error over the
elements above 1e-3 x max|reference|, the reference being the same loss through autograd in
float64 (tests/ppo_ref.ref64).  torch fp32 autograd is listed beside them.

Default: one JSON line per sample count, with rows as drawn and with rows kept 1e-3 away from the
clip edges (tests/ppo_ref.rows), the nets multiplied by --scale (default 1: as initialised).

--edge-rows: the measurement behind tests/test_gpu_learn_edges.py, per --scale (default 3 8) and
n in (5000, 33), on tests/ppo_ref.edge_case's nets and rows.  A `forward` block: max |d value| and
max |d log p| of fs_ppo_eval in each precision, and of torch fp32, against float64.  From it the
clip-edge margin of each (scale, precision): max(1e-3, 4 x the largest forward |d log p|) -- past
0.05 the run stops.  Then, on the rows at that margin, the gradient errors as above, each net's
largest, and the three loss means' |d| / max(1, |reference|), with torch fp32 on the same rows
beside them.  Written to --out (default profiles/r13a_learn_edges.json) and printed."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ppo_ref  # noqa: E402
from tests.ppo_ref import NAMES, nets, ref64, rows as make_rows, torch_reference  # noqa: E402
from footsies_gym_amd.ppo import PPOGrad  # noqa: E402

PRECISIONS = ("fp32", "split_bf16")
DEV = torch.device("cuda", 0)


def errs(got, ref):
    out = {}
    for name, g, e in zip(NAMES, got, ref):
        g, e = g.double().cpu(), e.double().cpu()
        scale = float(e.abs().max())
        d = (g - e).abs()
        big = e.abs() > 1e-3 * scale
        out[name] = [float(d.max()) / scale, float((d[big] / e.abs()[big]).max()) if bool(big.any()) else 0.0]
    return out


def net_max(e):
    """The largest max|d| / max|ref| over each network's tensors."""
    return {net: max(v[0] for k, v in e.items() if k.startswith(net)) for net in ("actor", "critic")}


def loss_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return [float(abs(g - r) / max(1.0, abs(r))) for g, r in zip(got, ref)]


def drawn_rows(scale):
    for n, margin in ((5000, 0.0), (70001, 0.0), (1_000_000, 0.0), (70001, 1e-3), (1_000_000, 1e-3)):
        actor, critic = nets(n % 7, device=DEV)
        with torch.no_grad():
            for p in list(actor.parameters()) + list(critic.parameters()):
                p.mul_(scale)
        rows = make_rows(actor, n, seed=n, margin=margin)
        ref, _, _, _ = ref64(actor, critic, rows, 0.2, 0.5, 0.01)
        t32, _ = torch_reference(actor, critic, rows, 0.2, 0.5, 0.01)
        res = {"n": n, "scale": scale, "clip_edge_margin": margin, "torch_fp32": errs(t32, ref)}
        for prec in PRECISIONS:
            pg = PPOGrad(actor, critic, precision=prec)
            pg(rows, 0.2, 0.5, 0.01)
            res[prec] = errs([p.grad.detach().clone() for p in pg.params], ref)
        torch.cuda.synchronize()
        print(json.dumps(res))


def forward_err(v, lp, ref_lp, ref_v):
    return {"values": float((v.double().cpu() - ref_v).abs().max()), "logp": float((lp.double().cpu() - ref_lp).abs().max()),
            "finite": bool(torch.isfinite(v).all()) and bool(torch.isfinite(lp).all()), "max_logp": float(lp.max())}


def edge_rows(scales, out_path):
    clip, vf, ent = ppo_ref.CLIP, ppo_ref.VF_COEF, ppo_ref.ENT_COEF
    sizes = (5000, 33)
    doc = {"tool": "tools/split_error.py --edge-rows", "actor_seed": ppo_ref.EDGE_SEED, "clip": clip, "vf_coef": vf,
           "ent_coef": ent, "reference": "float64 autograd (tests/ppo_ref.ref64)", "forward": [], "margin": [], "grad": []}
    for scale in scales:
        worst = {p: 0.0 for p in PRECISIONS}
        for n in sizes:
            actor, critic, table, (_, _, ref_lp, ref_v) = ppo_ref.edge_case(scale, n)
            a, c, t = ppo_ref.copy.deepcopy(actor).to(DEV), ppo_ref.copy.deepcopy(critic).to(DEV), table.to(DEV)
            x, act = t[:, :8].contiguous(), t[:, 8].to(torch.uint8).contiguous()
            with torch.no_grad():
                v32 = c(x).squeeze(-1)
                lp32 = torch.log_softmax(a(x), 1).gather(1, act.long()[:, None])[:, 0]
            rec = {"scale": scale, "n": n, "torch_fp32": forward_err(v32, lp32, ref_lp, ref_v)}
            for prec in PRECISIONS:
                v, lp = PPOGrad(a, c, precision=prec).evaluate(x, act, n)
                torch.cuda.synchronize()
                rec[prec] = forward_err(v, lp, ref_lp, ref_v)
                worst[prec] = max(worst[prec], rec[prec]["logp"])
            doc["forward"].append(rec)
            print(json.dumps(rec))
        for prec in PRECISIONS:
            margin = max(1e-3, 4 * worst[prec])
            doc["margin"].append({"scale": scale, "precision": prec, "forward_logp": worst[prec], "margin": margin})
            if not margin <= 0.05:
                raise SystemExit("scale %s %s: clip-edge margin %.3g exceeds 0.05 (the inside band is 0.4 wide)"
                                 % (scale, prec, margin))
            margin = math.ceil(margin * 1e4) / 1e4 if margin > 1e-3 else 1e-3  # (rounded up, as the test writes it)
            for n in sizes:
                actor, critic, table, (ref, ref_loss, _, _) = ppo_ref.edge_case(scale, n, margin)
                a, c, t = ppo_ref.copy.deepcopy(actor).to(DEV), ppo_ref.copy.deepcopy(critic).to(DEV), table.to(DEV)
                t32, l32 = torch_reference(a, c, t, clip, vf, ent)
                pg = PPOGrad(a, c, precision=prec)
                loss = pg(t, clip, vf, ent).clone()
                got = [p.grad.detach().clone() for p in pg.params]
                torch.cuda.synchronize()
                e, e32 = errs(got, ref), errs(t32, ref)
                rec = {"scale": scale, "n": n, "precision": prec, "margin": margin,
                       "finite": all(bool(torch.isfinite(g).all()) for g in got) and bool(torch.isfinite(loss).all()),
                       "kernel": e, "kernel_net_max": net_max(e), "kernel_loss": loss_err(loss, ref_loss),
                       "torch_fp32": e32, "torch_fp32_net_max": net_max(e32), "torch_fp32_loss": loss_err(l32, ref_loss),
                       "ref_loss": [float(v) for v in ref_loss]}
                doc["grad"].append(rec)
                print(json.dumps({k: v for k, v in rec.items() if k not in ("kernel", "torch_fp32")}))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=float, nargs="+", default=None, help="multiply every parameter of both nets")
    ap.add_argument("--edge-rows", action="store_true", help="tests/ppo_ref.edge_rows and the forward block")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13a_learn_edges.json"))
    args = ap.parse_args()
    if args.edge_rows:
        edge_rows([int(s) if s == int(s) else s for s in (args.scale or [3, 8])], args.out)
    else:
        for s in args.scale or [1.0]:
            drawn_rows(s)
