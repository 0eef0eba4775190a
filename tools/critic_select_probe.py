"""Best-of-k by the critic's score at the configs[4] shape (batch 32, 10
temperatures): scoring plus selection per batch on the new path against the
path a user had before it, and the streamed sweep with and without
``select="critic"``.  One GPU process per leg (run each under its own timeout).

  --leg score   new     D.score_labels (one stacked critic forward from the
                        int8 labels) + ops.sweep_select_score, then the host
                        copies of labels / best / score
                parent  per candidate a float one-hot and D(loc, vox, onehot)
                        in eval mode, the scores copied to the host, a host
                        loop over the buildings for the f64 means, a host
                        arg-max and an index gather
                host clock of one call ending in the result's host copies
                (both ends synchronise), alternated, median over REPS; and the
                device time of the new path between events
  --leg stream  InferenceSweep.run_stream over --graphs distinct buildings
                through the native loader, select=None and select="critic"
                alternated; --host-stacked: the k-copy CSR comes with the batch

  --critic-dtype both: --leg score alternates the f32 critic
                (D.score_labels + ops.sweep_select_score) and the f16 one
                (HalfCritic.select: one native call) in one process -- host
                clock ending in the host copies and device time between
                events, median over REPS -- and reports how often the two
                pick the same candidate; --leg stream adds a select="critic"
                pass with critic_dtype="f16" to each round

    python tools/critic_select_probe.py --leg score [--conv GATCONV] [--bce]      # JSON lines
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPS = 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=("score", "stream"))
    ap.add_argument("--graphs", type=int, default=3200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--taus", type=int, default=10)
    ap.add_argument("--dtype", default="f16", choices=("f16", "f32"))
    ap.add_argument("--conv", default="GATCONV", choices=("GATCONV", "GATV2CONV"))
    ap.add_argument("--bce", action="store_true", help="USE_WGANGP = False: the Sigmoid critic")
    ap.add_argument("--critic-dtype", default="f32", choices=("f32", "both"),
                    help="both: the f16 critic scorer next to the f32 one, alternated")
    ap.add_argument("--workers", type=int, default=2)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-stacked", action="store_true",
                    help="the loader's collate builds the k-copy stacked CSR and uploads it with the batch "
                         "(prepare copies) instead of CSR.stacked's device ops per batch")
    args = ap.parse_args()
    from vgan import ops
    from vgan.config import Configuration
    from vgan.infer import InferenceSweep, geometric_taus
    from vgan.loader import GraphLoader
    from vgan.models import VoxelGNNDiscriminator, VoxelGNNGenerator
    from vgan.store import write_store
    from vgan.synth import SyntheticDataset

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    graphs = args.graphs if args.leg == "stream" else args.batch
    store = write_store(os.path.join(tempfile.mkdtemp(prefix="vgan_critic_select_"), "store"),
                        SyntheticDataset(graphs, seed=2024))
    cfg = Configuration()
    cfg.DEVICE = str(dev)
    cfg.runtime["rng"] = "device"
    cfg.USE_WGANGP = not args.bce
    cfg.DISCRIMINATOR_CONV_TYPE = args.conv
    torch.manual_seed(cfg.SEED)
    G = VoxelGNNGenerator(cfg, 17, 12)
    D = VoxelGNNDiscriminator(cfg, 17, 12)
    K = cfg.NUM_CLASSES
    taus = geometric_taus(1.0, 0.1, args.taus)

    def loader(idx=None):
        return GraphLoader(store, idx, batch_size=args.batch, shuffle=False, device=dev, prefetch=4,
                           prepare=(K, (args.taus,) if args.host_stacked else ()), workers=args.workers)

    sw = InferenceSweep(G, taus, dtype=args.dtype, critic=D)
    both = args.critic_dtype == "both"
    sw16 = InferenceSweep(G, taus, dtype=args.dtype, critic=D, critic_dtype="f16") if both else None
    if args.leg == "stream":
        # (sweep, select, the name printed)
        legs = [(sw, None, None), (sw, "critic", "critic")] + ([(sw16, "critic", "critic_f16")] if both else [])
        for s_, select, _ in legs[1:]:
            s_.run_stream(loader(list(range(4 * args.batch))), select=select)  # warm-up
        torch.cuda.synchronize()
        rates = {name: [] for _, _, name in legs}
        ms = {name: [] for _, _, name in legs}
        for _ in range(args.passes):
            for s_, select, name in legs:
                t0 = time.perf_counter()
                res = s_.run_stream(loader(), select=select)
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                rates[name].append(res["samples"] / el)
                ms[name].append(el / res["batches"] * 1e3)
        for _, _, select in legs:
            print(json.dumps({"leg": "stream", "dtype": args.dtype, "select": select, "workers": args.workers,
                              "host_stacked": args.host_stacked, "conv": args.conv, "wgangp": cfg.USE_WGANGP,
                              "batches": res["batches"],
                              "samples_per_s_median": round(statistics.median(rates[select]), 1),
                              "samples_per_s_all": [round(r, 1) for r in rates[select]],
                              "ms_per_batch_median": round(statistics.median(ms[select]), 4)}), flush=True)
        return

    loc, vox = next(iter(loader(list(range(args.batch)))))
    pred = sw.run_batch(loc, vox).clone()
    ptr = vox.ptr
    k, n = pred.shape
    g = vox.num_graphs
    ptr_h = ptr.cpu().numpy()
    batch_h = np.repeat(np.arange(g), np.diff(ptr_h))
    D.eval()
    torch.cuda.synchronize()

    def new():
        return ops.sweep_select_score(D.score_labels(loc, vox, pred), pred, ptr)

    def new_host():
        s = new()
        return {f: getattr(s, f).cpu() for f in ("labels", "best", "score")}

    def parent():
        with torch.no_grad():
            rows = [D(loc, vox, torch.nn.functional.one_hot(pred[c].long(), K).float()).reshape(-1) for c in range(k)]
        s = torch.stack(rows).cpu().numpy().astype(np.float64)
        pred_h = pred.cpu().numpy()
        score = np.empty((k, g))
        for b in range(g):  # the host loop over buildings
            score[:, b] = s[:, ptr_h[b]:ptr_h[b + 1]].mean(axis=1)
        best = np.argmax(score, axis=0)
        return pred_h[best[batch_h], np.arange(n)], best, score

    if both:
        score_f16_vs_f32(sw16.half_critic, new, new_host, loc, vox, pred, shape={
            "copies": k, "rows": n, "buildings": g, "classes": K, "conv": args.conv, "wgangp": cfg.USE_WGANGP})
        return
    for _ in range(5):
        got, ref = new_host(), parent()
    torch.cuda.synchronize()
    err = float(np.abs(got["score"].numpy() - ref[2]).max())
    gaps = np.sort(ref[2], axis=0)
    agree = float((got["best"].numpy() == ref[1]).mean())
    dev_ms = []
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(REPS):
        a.record()
        new()
        e.record()
        torch.cuda.synchronize()
        dev_ms.append(a.elapsed_time(e))
    host_new, host_parent = [], []
    for _ in range(REPS):  # alternated
        t0 = time.perf_counter()
        new_host()
        host_new.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        parent()
        host_parent.append((time.perf_counter() - t0) * 1e3)
    shape = {"copies": k, "rows": n, "buildings": g, "classes": K, "conv": args.conv, "wgangp": cfg.USE_WGANGP}
    print(json.dumps({"leg": "new", "shape": shape, "reps": REPS,
                      "ms_median": round(statistics.median(host_new), 3),
                      "ms_min_max": [round(min(host_new), 3), round(max(host_new), 3)],
                      "events_ms_median": round(statistics.median(dev_ms), 3),
                      "max_abs_mean_difference_to_parent": err, "best_agreement": round(agree, 4),
                      "smallest_top_two_gap": float((gaps[-1] - gaps[-2]).min()) if k > 1 else None}), flush=True)
    print(json.dumps({"leg": "parent", "critic_forwards": k, "reps": REPS,
                      "ms_median": round(statistics.median(host_parent), 3),
                      "ms_min_max": [round(min(host_parent), 3), round(max(host_parent), 3)]}), flush=True)


def score_f16_vs_f32(hc, f32_dev, f32_host, loc, vox, pred, shape):
    """Scoring plus selection of one batch by the f32 and the f16 critic, alternated."""

    def f16_dev():
        return hc.select(loc, vox, pred)

    def f16_host():
        s = f16_dev()
        return {f: getattr(s, f).cpu() for f in ("labels", "best", "score")}

    for _ in range(5):
        a, b = f32_host(), f16_host()
    torch.cuda.synchronize()
    sa, sb = a["score"].numpy(), b["score"].numpy()
    top = np.sort(sa, axis=0)
    ev = {"f32": [], "f16": []}
    host = {"f32": [], "f16": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(REPS):  # alternated
        for name, fn_dev, fn_host in (("f32", f32_dev, f32_host), ("f16", f16_dev, f16_host)):
            e0.record()
            fn_dev()
            e1.record()
            torch.cuda.synchronize()
            ev[name].append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            fn_host()
            host[name].append((time.perf_counter() - t0) * 1e3)
    for name in ("f32", "f16"):
        print(json.dumps({"leg": "score", "critic_dtype": name, "shape": shape, "reps": REPS,
                          "ms_median": round(statistics.median(host[name]), 3),
                          "ms_min_max": [round(min(host[name]), 3), round(max(host[name]), 3)],
                          "events_ms_median": round(statistics.median(ev[name]), 3)}), flush=True)
    print(json.dumps({"leg": "score", "f16_vs_f32": {
        "best_agreement": round(float((a["best"].numpy() == b["best"].numpy()).mean()), 4),
        "buildings": int(a["best"].numel()),
        "max_abs_mean_difference": float(np.abs(sa - sb).max()),
        "smallest_top_two_gap_f32": float((top[-1] - top[-2]).min()) if sa.shape[0] > 1 else None,
        "top_two_gap_of_disagreeing_buildings": [float(x) for x in (top[-1] - top[-2])[
            a["best"].numpy() != b["best"].numpy()]]}}), flush=True)


if __name__ == "__main__":
    main()
