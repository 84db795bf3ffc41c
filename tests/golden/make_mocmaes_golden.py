#!/usr/bin/env python3
"""Extract the MOCMAES golden data from the reference's committed generation files.

Source: <korali root>/tests/python/plot/mocmaes/gen00000{000,010,...,350}.json,
36 full solver states (one every 10 generations) of a run of
examples/optimization/multiobjective/run-mocmaes.py's setup at dim 3
(N = 3, P = 32, mu = 16, K = 2, bounds +-25, 'Initial Standard Deviation' 3,
objective negative_rosenbrock_and_sphere), written by the reference's
Experiment::saveState.  Data only: every solver field (both generators' GSL
states in 'Range'), the variables, the seeds and 'Is Finished'.  Written
gzip-compressed: tests/mocmaes_ref.py load_golden() reads it.

The files were written by an older MOCMAES than the snapshot's
(MOCMAES.cpp.base): it fills the parent slots in ascending index of the merged
population instead of 'values.size() - sortedIndices[i] - 1' (:385), and names
'Previous Best Variables Vector' 'Previous Best Variables'.

Re-run:  python3 tests/golden/make_mocmaes_golden.py <korali root>
"""
import gzip
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))


def main(root):
    src = os.path.join(root, "tests", "python", "plot", "mocmaes")
    states = []
    rows, index = [], {}
    for g in range(0, 351, 10):
        with open(os.path.join(src, "gen%08d.json" % g)) as f:
            j = json.load(f)
        sv = j["Solver"]
        archive = []
        for x, f in zip(sv.pop("Sample Collection"), sv.pop("Sample Value Collection")):
            key = json.dumps([x, f])
            if key not in index:
                index[key] = len(rows)
                rows.append([x, f])
            archive.append(index[key])
        sv["Archive"] = archive
        states.append({"Current Generation": j["Current Generation"], "Is Finished": j["Is Finished"],
                       "Random Seed": j["Random Seed"], "Variables": j["Variables"], "Solver": sv})
    text = json.dumps({"source": "tests/python/plot/mocmaes", "archive rows": rows, "states": states}, separators=(",", ":")) + "\n"
    with open(os.path.join(OUT, "mocmaes_golden.json.gz"), "wb") as raw:  # (no name, no time: the same bytes every run)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())


if __name__ == "__main__":
    main(sys.argv[1])
