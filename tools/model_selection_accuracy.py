"""Every error ratio that tests/test_gpu_model_selection.py measures (per rung, path and precision), from one run of that
file with -s on an MI355X: the tests print one `measured {...}` line per figure before they assert.  Writes the list, and
the suite's outcome, as one JSON document.

Usage: python tools/model_selection_accuracy.py [out.json]      (default: profiles/model_selection_accuracy.json)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "model_selection_accuracy.json")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_model_selection.py"), "-m", "gpu",
                        "-s", "-q", "-p", "no:cacheprovider"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = r.stdout.decode(errors="replace")
    rows = [json.loads(ln.split("measured ", 1)[1]) for ln in text.splitlines() if "measured {" in ln]
    summary = [ln for ln in text.splitlines() if " passed" in ln or " failed" in ln][-1:]
    with open(out, "w") as f:
        json.dump({"tool": "model_selection_accuracy", "pytest_exit": r.returncode, "pytest_summary": summary,
                   "unit_roundoff": {"f64": 2.0 ** -53, "f32": 2.0 ** -24}, "measured": rows}, f, indent=1)
        f.write("\n")
    sys.stdout.write(text[-3000:])
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
