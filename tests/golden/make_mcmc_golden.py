#!/usr/bin/env python3
"""Extract the MCMC golden data from the reference's committed generation files.

Source: <korali root>/tests/python/plot/mcmc/gen0000{0000,0500,...,5500}.json,
a complete run of Sampler/MCMC on a Sampling problem (one variable, Burn In
500, 5000 samples; the model of tests/python/plot is -0.5 * x * x) written by
the reference's Experiment::saveState.  Data only: the solver's configuration,
the two generator seeds, the last file's Sample Database, Sample Evaluation
Database and generator states ('Range', GSL's 5000 bytes in hex), and for each
of the 12 recorded generations the scalar and vector fields of the solver.
Written gzip-compressed: tests/mcmc_ref.py load_golden() reads it.

Re-run:  python3 tests/golden/make_mcmc_golden.py <korali root>
"""
import gzip
import json
import os
import sys

OUT = os.path.dirname(os.path.abspath(__file__))

CONFIG = ["Burn In", "Leap", "Rejection Levels", "Use Adaptive Sampling", "Non Adaption Period",
          "Chain Covariance Scaling"]
FIELDS = ["Acceptance Count", "Acceptance Rate", "Proposed Sample Count", "Chain Length", "Model Evaluation Count",
          "Chain Leader", "Chain Leader Evaluation", "Chain Candidate", "Chain Candidates Evaluations", "Chain Mean",
          "Chain Covariance", "Chain Covariance Placeholder", "Cholesky Decomposition Covariance",
          "Cholesky Decomposition Chain Covariance"]


def main(root):
    src = os.path.join(root, "tests", "python", "plot", "mcmc")
    gens = []
    for g in range(0, 5501, 500):
        with open(os.path.join(src, "gen%08d.json" % g)) as f:
            j = json.load(f)
        sv = j["Solver"]
        rec = {"Current Generation": j["Current Generation"], "Database Size": len(sv["Sample Database"])}
        rec.update({k: sv[k] for k in FIELDS})
        gens.append(rec)
        if g == 0:
            first = j
        last = j
    sv0, sv = first["Solver"], last["Solver"]
    out = {
        "source": "tests/python/plot/mcmc",
        "Configuration": {k: sv0[k] for k in CONFIG},
        "Max Samples": sv0["Termination Criteria"]["Max Samples"],
        "Variables": [{k: v[k] for k in ("Name", "Initial Mean", "Initial Standard Deviation")}
                      for v in first["Variables"]],
        "Normal Seed": sv0["Normal Generator"]["Random Seed"],
        "Uniform Seed": sv0["Uniform Generator"]["Random Seed"],
        "generations": gens,
        "Sample Database": sv["Sample Database"],
        "Sample Evaluation Database": sv["Sample Evaluation Database"],
        "Normal Generator Range": sv["Normal Generator"]["Range"],
        "Uniform Generator Range": sv["Uniform Generator"]["Range"],
    }
    text = json.dumps(out, separators=(",", ":")) + "\n"
    with open(os.path.join(OUT, "mcmc_golden.json.gz"), "wb") as raw:  # (no name, no time: the same bytes every run)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(text.encode())


if __name__ == "__main__":
    main(sys.argv[1])
