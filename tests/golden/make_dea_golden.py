#!/usr/bin/env python3
"""Extract the DEA golden data from the reference's committed generation files.

Source: <korali root>/tests/python/plot/dea/gen000000{00..23}.json, the full
per-generation solver states of examples/optimization/stochastic/run-dea.py
written by the reference's Experiment::saveState.  Data only: every solver
field, the variables, the seeds, 'Is Finished' and 'Results'.  The Uniform
Generator's 'Range' (its GSL state) is kept for every generation, the Normal
Generator's (never drawn from, so constant) only for generation 1.  Written
gzip-compressed (0.66 MB of JSON): tests/dea_ref.py load_golden() reads it.

Re-run:  python3 tests/golden/make_dea_golden.py <korali root>
"""
import gzip
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))


def main(root):
    src = os.path.join(root, "tests", "python", "plot", "dea")
    gens = []
    for g in range(24):
        with open(os.path.join(src, "gen%08d.json" % g)) as f:
            j = json.load(f)
        sv = j["Solver"]
        if g != 1:
            del sv["Normal Generator"]["Range"]
        keep = {"Current Generation": j["Current Generation"], "Is Finished": j["Is Finished"],
                "Random Seed": j["Random Seed"], "Variables": j["Variables"], "Solver": sv}
        if "Results" in j:
            keep["Results"] = j["Results"]
        gens.append(keep)
    text = json.dumps({"source": "tests/python/plot/dea", "generations": gens}, separators=(",", ":")) + "\n"
    with open(os.path.join(OUT, "dea_golden.json.gz"), "wb") as raw:  # (no name, no time: the same bytes every run)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())


if __name__ == "__main__":
    main(sys.argv[1])
