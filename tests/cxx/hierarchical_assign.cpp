// An Experiment as a JSON value in the C++ API, as the hierarchical problems
// take their sub-experiments: e["Problem"]["Sub Experiments"][i] = sub.
#include <cstdio>

#include "korali.hpp"

int main() {
  korali::Experiment sub;
  sub["Is Finished"] = true;
  sub["Solver"]["Sample LogPrior Database"] = std::vector<double>{-1.0, -2.0, -3.0};
  korali::Experiment e;
  e["Problem"]["Type"] = "Hierarchical/Psi";
  e["Problem"]["Sub Experiments"][0] = sub;
  e["Problem"]["Sub Experiments"][1] = sub;
  e["Problem"]["Psi Experiment"] = sub;
  sub["Is Finished"] = false;  // the value stored is a copy
  korali::Json &first = e["Problem"]["Sub Experiments"][0];
  std::vector<double> lp = first["Solver"]["Sample LogPrior Database"];
  const bool ok = e["Problem"]["Sub Experiments"].size() == 2 && first["Is Finished"] == true && lp.size() == 3 &&
                  lp[2] == -3.0 && e["Problem"]["Psi Experiment"]["Is Finished"] == true;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
