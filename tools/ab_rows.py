#!/usr/bin/env python3
"""Same-box A/B of two builds of the library (NMPC_HIP_LIBRARY) on a few bench rows, interleaved.
usage: ab_rows.py <libA.so> <libB.so> [rounds]
       ab_rows.py --bench [--family F] [--out FILE.json] <libA.so> <libB.so> [rounds]
--bench: each run is the plain benchmark command (python bench.py --gpus 1 --steps 5 --warmup 1 [--family F]) in a process of
its own, A and B in turn; prints one line per run and, at the end, both series, their medians, the ratio B / A of the medians
and whether the series overlap (a gain is only claimed where every run of B beats every run of A). Stops at the first run
that fails or exceeds its time limit."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = r'''
import json, os, sys
sys.path.insert(0, %r)
import bench
class A: gpus = 1
env = bench.Env(A())
for wl, fam, st in (("cfg2", "toward_robot", 3), ("cfg2", "passing", 3), ("cfg1", "toward_robot", 8)):
    r = bench.run_workload(env, wl, fam, "f32", st, 1)
    print(json.dumps({"lib": os.path.basename(os.environ.get("NMPC_HIP_LIBRARY", "default")), "row": wl + " " + fam, "solves_per_s": round(r["value"]), "kernel_ms": round(r["roofline"]["kernel_ms"], 2)}), flush=True)
''' % ROOT


def plain_bench(args):
    family, out = "toward_robot", None
    while args and args[0].startswith("--"):
        k = args.pop(0)
        if k == "--family":
            family = args.pop(0)
        elif k == "--out":
            out = args.pop(0)
    libs = [os.path.abspath(a) for a in args[:2]]
    rounds = int(args[2]) if len(args) > 2 else 5
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1"] + (["--family", family] if family != "toward_robot" else [])
    series = {lib: [] for lib in libs}
    for rnd in range(rounds):
        for lib in libs:
            p = subprocess.run(cmd, env=dict(os.environ, NMPC_HIP_LIBRARY=lib), capture_output=True, text=True, timeout=300)
            line = next((l for l in p.stdout.splitlines() if l.startswith("{")), None)
            if p.returncode != 0 or line is None:
                sys.exit(f"run failed (rc {p.returncode}): {p.stderr[-800:]}")
            r = json.loads(line)
            series[lib].append({"solves_per_s": r["value"], "ms_per_step": r["ms_per_step"]})
            print(json.dumps({"round": rnd, "lib": os.path.basename(lib), **series[lib][-1]}), flush=True)
    a, b = ([x["solves_per_s"] for x in series[lib]] for lib in libs)
    res = {"command": " ".join(["python", "bench.py"] + cmd[2:]), "family": family, "rounds": rounds, "order": "A, B in turn, one process per run",
           "A": {"lib": os.path.basename(libs[0]), "runs": series[libs[0]], "median_solves_per_s": statistics.median(a)},
           "B": {"lib": os.path.basename(libs[1]), "runs": series[libs[1]], "median_solves_per_s": statistics.median(b)},
           "ratio_B_over_A_of_medians": statistics.median(b) / statistics.median(a),
           "A_spread_rel": (max(a) - min(a)) / statistics.median(a), "B_spread_rel": (max(b) - min(b)) / statistics.median(b),
           "every_B_run_faster_than_every_A_run": min(b) > max(a), "every_B_run_slower_than_every_A_run": max(b) < min(a)}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--bench":
        plain_bench(sys.argv[2:])
        sys.exit(0)
    libs = [os.path.abspath(a) for a in sys.argv[1:3]]
    for rnd in range(int(sys.argv[3]) if len(sys.argv) > 3 else 2):
        for lib in libs:
            out = subprocess.run([sys.executable, "-c", CODE], env=dict(os.environ, NMPC_HIP_LIBRARY=lib), capture_output=True, text=True)
            sys.stdout.write("".join(l + "\n" for l in out.stdout.splitlines() if l.startswith("{")) or out.stderr[-800:])
            sys.stdout.flush()
