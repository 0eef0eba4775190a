"""The BCE step (USE_WGANGP = False) with the HIP engines and with autograd.

usage: python tools/bce_probe.py [--steps 50] [--rounds 3] [--out FILE]

The batch is bench.py's first pooled one (configs[1]: 32 synthetic buildings,
f32).  Two trainers from the same seed -- runtime critic / gen "engine"
(vgan/bce.py, vgan/genstep.py) and "autograd" (the torch-op branches of
Trainer._compute_discriminator_loss / _compute_generator_loss) -- each replay
their captured step (step_graphed); the legs alternate in one process,
``rounds`` times ``steps`` steps each, every step timed with device events.
Then one eager step of each under torch.profiler counts its dispatches
(kernel launches, memsets and copies: what the captured graph replays).
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from collections import Counter

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "building-gan-graph-conditioned-architectural-volume-generation_amd"))


def build(bench, mode: str, dev):
    from vgan.config import Configuration

    cfg = Configuration()
    cfg.DEVICE = str(dev)
    cfg.USE_WGANGP = False
    cfg.runtime["rng"] = "device"
    cfg.runtime["critic"] = cfg.runtime["gen"] = mode
    return bench.build_trainer(cfg, "f32")


def timed_steps(step, steps: int):
    """Per-step device milliseconds of ``steps`` back-to-back calls."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for s in range(steps):
        step()
        evs[s + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def dispatches(step) -> int:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU
                    and e.name.startswith(("hip", "cuda")))
    return sum(c for n, c in names.items() if "Launch" in n or "Memset" in n or "Memcpy" in n)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from vgan.bce import BceCriticEngine
    from vgan.config import Configuration

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    loc, vox = bench.make_pool(Configuration(), 0, 1, 1, 32, dev)[0]
    legs = {m: build(bench, m, dev) for m in ("engine", "autograd")}
    assert isinstance(legs["engine"].critic, BceCriticEngine) and legs["engine"].gen_engine is not None
    assert legs["autograd"].critic is None and legs["autograd"].gen_engine is None
    res = {"rows": vox.num_nodes, "steps": args.steps, "rounds": args.rounds, "legs": {}}
    for m, tr in legs.items():  # capture and warm every leg before any timing
        for _ in range(5):
            out = tr.step_graphed(loc, vox)
        torch.cuda.synchronize()
        res["legs"][m] = {"d_loss": round(float(out["d_losses"][-1]), 6), "g_loss": round(float(out["g_loss"]), 6),
                          "ms": []}
    for _ in range(args.rounds):  # alternate the legs
        for m, tr in legs.items():
            res["legs"][m]["ms"].append(timed_steps(lambda: tr.step_graphed(loc, vox), args.steps))
    for m, tr in legs.items():
        leg = res["legs"][m]
        medians = [statistics.median(r) for r in leg["ms"]]
        leg["median_ms_per_round"] = [round(v, 4) for v in medians]
        leg["median_ms"] = round(statistics.median(v for r in leg["ms"] for v in r), 4)
        leg["ms"] = [[round(v, 4) for v in r] for r in leg["ms"]]
        tr.step(loc, vox)  # eager once (lazy initialisation), then counted
        leg["dispatches_per_step"] = dispatches(lambda: tr.step(loc, vox))
    res["engine_over_autograd"] = round(res["legs"]["engine"]["median_ms"] / res["legs"]["autograd"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
