"""Which kernels the W4A4 GEMM entry points launch, case by case: runs every case of tests/gemm_route_cases.py once, a one-element fill
in front of each as a marker, and condenses a kernel trace of that run into the ordered list of (kernel, grid, workgroup, LDS bytes)
per case -- the file two commits must agree on when only host code changed between them (profiles/gemm_routes/).

    rocprofv3 --kernel-trace --output-format csv -d RAW -o routes -- python tools/gemm_routes.py
    python tools/gemm_routes.py --summarize RAW OUT.txt"""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    import torch
    from tests import gemm_route_cases as C
    marker = torch.empty(1, dtype=torch.float32, device="cuda")
    for i, case in enumerate(C.CASES):
        marker.fill_(float(i))
        torch.cuda.synchronize()
        print(case[0], C.run(case)[:16], flush=True)


def summarize(raw, out):
    from tests import gemm_route_cases as C
    files = glob.glob(os.path.join(raw, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    case, lines = -1, []
    for r in rows:
        name = r["Kernel_Name"]
        if "FillFunctor" in name:
            case += 1
            lines.append(f"== {C.CASES[case][0]}")
        elif not name.startswith("__amd_rocclr"):               # (the runtime's own copy / fill kernels)
            grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
            wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
            lines.append(f"   {name}  grid {grid}  workgroup {wg}  lds {r.get('LDS_Block_Size', r.get('Group_Segment_Size'))}")
    assert case == len(C.CASES) - 1, (case, len(C.CASES))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(len(lines) - len(C.CASES), "launches in", len(C.CASES), "cases ->", out)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        run()
