"""Per-case comparison of an A/B of scripts/bench_corr_dense.py and scripts/bench_corr1d.py: each script run for a parent
build and a new build alternately, twice, in one session on one machine (result files DIR/<script>.parent1.json,
.parent2.json, .<cand>1.json, .<cand>2.json).

    python scripts/compare_corr_ab.py DIR CAND OUT.json

Per (case, kernel): noise = |parent run 1 - parent run 2| of the medians.  A case is within noise when the mean of the
candidate's two medians exceeds the mean of the parent's two by no more than that noise.  The stricter figure, the
candidate's worse run against the parent's better one, is recorded beside it.  OUT.json holds the eight result files, the
per-case comparison, the cases outside noise and the worst ratio; a summary per script and kernel goes to stdout.
"""
import json
import statistics
import sys

SCRIPTS = (("bench_corr_dense", ("auto", "direct")), ("bench_corr1d", ("tiled", "general")))
RULE = ("within_noise: mean of the new build's two medians - mean of the parent's two medians <= |parent run 1 - parent run 2| "
        "of the same case in the same session; new_worst_minus_parent_best_us is the stricter figure, recorded but not the rule")


def compare(p1, p2, c1, c2):
    noise = abs(p1 - p2)
    mean_diff = (c1 + c2) / 2 - (p1 + p2) / 2
    return {"parent_us": [p1, p2], "new_us": [c1, c2], "noise_us": round(noise, 2),
            "new_worst_minus_parent_best_us": round(max(c1, c2) - min(p1, p2), 2), "mean_diff_us": round(mean_diff, 2),
            "mean_ratio": round((c1 + c2) / (p1 + p2), 4), "within_noise": mean_diff <= noise}


def main():
    d, cand, out = sys.argv[1:4]
    names = ("parent1", "parent2", cand + "1", cand + "2")
    res = {"rule": RULE, "runs": {}, "cases": {}}
    for script, kernels in SCRIPTS:
        runs = {n: json.load(open(f"{d}/{script}.{n}.json")) for n in names}
        res["runs"][script] = runs
        for case in runs["parent1"]["cases"]:
            for k in kernels:
                res["cases"][f"{script}:{case}:{k}"] = compare(*(runs[n]["cases"][case][k]["median_us"] for n in names))
    worst = max(res["cases"], key=lambda c: res["cases"][c]["mean_ratio"])
    res["worst_case"] = {worst: res["cases"][worst]}
    res["outside_noise"] = sorted(c for c, v in res["cases"].items() if not v["within_noise"])
    with open(out, "w") as f:
        json.dump(res, f, indent=1)

    print(len(res["cases"]), "cases;", len(res["outside_noise"]), "outside noise; worst", worst, res["cases"][worst])
    for c in sorted(res["outside_noise"], key=lambda c: -res["cases"][c]["mean_ratio"]):
        print(" ", c, res["cases"][c])
    for script, kernels in SCRIPTS:
        for k in kernels:
            rs = [v["mean_ratio"] for c, v in res["cases"].items() if c.startswith(script + ":") and c.endswith(":" + k)]
            print(script, k, len(rs), "cases, new / parent: geomean", round(statistics.geometric_mean(rs), 4), "min", min(rs), "max", max(rs))
    return 0


if __name__ == "__main__":
    sys.exit(main())
