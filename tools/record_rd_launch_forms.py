"""Record the launch form of the decision kernel for the cases of tests/rd_plan_cases.py: one real launch each on tiny pictures, the string hevcdl_last_rd_launch
reports, into tests/golden/rd_launch_forms.json (the device's CU count and the builds' wavefronts per workgroup in the header).  The file is the authority tests/test_rd_plan.py and
tests/test_rd_gpu.py::test_launch_forms_are_the_recorded_ones hold the launch plan to, so it is recorded with the library of the commit BEFORE a change of the plan:
    HEVCDL_LIB=<that commit's lib/libhevcdl_hip.so> python tools/record_rd_launch_forms.py [OUT.json]
Needs a GPU; takes seconds."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import rd_plan_cases


def main(out):
    case_list = rd_plan_cases.cases()
    cus = rd_plan_cases.device_cus()
    launches = rd_plan_cases.run_cases(case_list)
    for c in case_list:
        c["launch"] = launches[c["name"]]
        print("%-28s %s" % (c["name"], c["launch"]))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"cus": cus, "waves": rd_plan_cases.build_waves(), "cases": case_list}, f, indent=1)
        f.write("\n")
    print("%d cases on %d CUs -> %s" % (len(case_list), cus, out))
    rd_plan_cases.check_coverage(launches)      # every form, every build, every pair either side of its threshold: otherwise move the counts


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rd_launch_forms.json"))
