"""The rows and verdicts of a parent / result alternation.

A visit leaves one file of JSON lines per run in a directory, named
<tool>_P<i>.jsonl for the parent commit's runs and <tool>_R<i>.jsonl for the
result's (i = 1, 2, 3: P1 R1 P2 R2 P3 R3 in time): the output of bench.py or of
a tools/bench_sharded_*.py run. Every timed figure of a line (each
`median_us`, each `*_host_enqueue_us`, bench.py's `value` and `ms_per_step`)
is one row, and the rule per row is

    |median(result) - median(parent)| <= max(parent) - min(parent).

    python tools/alternating_table.py RUNS_DIR [MORE_DIRS ...] --out profiles/<name>/alternating.json

writes the rows to the JSON file and prints the markdown table."""
import argparse
import glob
import json
import os
import re
import statistics

TIMED = ("median_us", "value", "ms_per_step")


def leaves(row, prefix=""):
    for k, v in row.items():
        if isinstance(v, dict):
            yield from leaves(v, prefix + k + " / ")
        elif isinstance(v, (int, float)) and not isinstance(v, bool) and (
                k in TIMED or k.endswith("host_enqueue_us")):
            yield prefix + k, float(v)


def figures(path):
    out = {}
    for line in open(path):
        line = line.strip()
        if not line.startswith("{"):
            continue
        row = json.loads(line)
        what = str(row.get("what", row.get("metric", "line")))
        if len(what) > 60:
            what = what[:60].rstrip() + "..."
        tag = what + (" [%s]" % row["dtype"] if "dtype" in row else "")
        for k, v in leaves(row):
            out[tag + " / " + k] = v
    return out


def rows_of(directory):
    tools = sorted({re.sub(r"_[PR]\d\.jsonl$", "", os.path.basename(f))
                    for f in glob.glob(os.path.join(directory, "*_[PR][123].jsonl"))})
    for tool in tools:
        runs = {t: [figures(os.path.join(directory, "%s_%s%d.jsonl" % (tool, t, i)))
                    for i in (1, 2, 3)] for t in "PR"}
        for key in runs["P"][0]:
            if not all(key in r for r in runs["P"] + runs["R"]):
                continue
            p, r = [x[key] for x in runs["P"]], [x[key] for x in runs["R"]]
            spread, d = max(p) - min(p), statistics.median(r) - statistics.median(p)
            yield {"tool": tool, "what": key, "parent": p, "result": r,
                   "parent_spread": round(spread, 4), "result_minus_parent": round(d, 4),
                   "within_spread": abs(d) <= spread,
                   # bench.py's `value` is a rate: higher is better
                   "result_slower_beyond_spread": (-d if key.endswith("/ value") else d) > spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("runs", nargs="+", help="directories of <tool>_{P,R}{1,2,3}.jsonl")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    rows = [row for d in args.runs for row in rows_of(d)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"unit": "us, median of one run (bench.py: the line's own unit)",
                   "order": "parent, result alternating, three times per tool, one GPU visit",
                   "rule": "|median(result) - median(parent)| <= max(parent) - min(parent)",
                   "rows": rows}, f, indent=1)
        f.write("\n")
    print("| tool, row | P | R | P's spread | R − P | within |\n|---|---|---|---|---|---|")
    def num(a, sign=""):
        return ("%" + sign + ".4g" if abs(a) < 100 else "%" + sign + ".1f") % a

    for x in rows:
        print("| %s, %s | %s | %s | %s | %s | %s |" % (
            x["tool"], x["what"], ", ".join(map(num, x["parent"])),
            ", ".join(map(num, x["result"])), num(x["parent_spread"]),
            num(x["result_minus_parent"], "+"), "yes" if x["within_spread"] else "no"))
    outside = [x for x in rows if not x["within_spread"]]
    print("\n%d of %d rows outside the rule" % (len(outside), len(rows)))


if __name__ == "__main__":
    main()
