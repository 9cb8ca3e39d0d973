#!/usr/bin/env python3
"""profiles/conditioning_ladder.json from the output of ONE GPU run of the conditioning ladder:
    python -m pytest tests/test_gpu_breakdown.py -m gpu -q -s -k conditioning_ladder > ladder.log
    python tools/ladder_json.py ladder.log
Every "LADDER {json}" line the tests print becomes one record (figures rounded to three digits): per problem, rung, path
and precision the device's figures beside those of the references on the same rung."""
import json
import os
import sys


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = []
    for line in open(sys.argv[1]):
        at = line.find("LADDER {")
        if at < 0:
            continue
        rec = json.loads(line[at + 7:])
        rows.append({k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in rec.items()})
    rows.sort(key=lambda r: (r["dtype"], r["problem"], r["path"], -r["sigma2"], r.get("multi_column", -1)))
    with open(os.path.join(root, "profiles", "conditioning_ladder.json"), "w") as fh:
        fh.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print("%d records" % len(rows))


if __name__ == "__main__":
    main()
