"""Hold the device planner's arithmetic (csrc/augment.hip plan_row, host-callable) against preprocess.resize_plan without a GPU:
compiles a stand-alone program around plan_row, runs it on the CPU for a sweep of extents and output sizes, both filters, and
compares bounds, taps and the zero padding with the host planner bit for bit.  (On the device the same comparison is
tests/test_gpu_train_transform.py::test_planner_tables_equal_the_host_plan_bitwise.)

  python tools/plan_host_check.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openvision_amd.augment import max_taps            # noqa: E402
from openvision_amd.build import FLAGS, hipcc          # noqa: E402
from openvision_amd.preprocess import resize_plan      # noqa: E402

MAIN = r"""
#include "%s"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {          // cubic in out max_taps -> one line per output position: first count taps...
    const int cubic = atoi(argv[1]), in = atoi(argv[2]), out = atoi(argv[3]), mt = atoi(argv[4]);
    std::vector<int> b(2), t(mt);
    for (int xx = 0; xx < out; ++xx) {
        if (cubic) plan_row<true>(in, out, xx, mt, b.data(), t.data());
        else plan_row<false>(in, out, xx, mt, b.data(), t.data());
        printf("%%d %%d", b[0], b[1]);
        for (int x = 0; x < mt; ++x) printf(" %%d", t[x]);
        printf("\n");
    }
    return 0;
}
"""


def main():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "plan_host.hip"), os.path.join(tmp, "plan_host")
        with open(src, "w") as f:
            f.write(MAIN % os.path.join(ROOT, "openvision_amd", "csrc", "augment.hip"))
        subprocess.run([hipcc()] + [x for x in FLAGS if x != "-fPIC"] + ["-o", exe, src], check=True)
        bad = n = 0
        for interp in ("bilinear", "bicubic"):
            for out in (7, 32, 224):
                for ext in list(range(1, 70)) + [77, 333, 480, 481, 500, 640, 641, 1000, 2047]:
                    hb, hk, ks = resize_plan(ext, out, interp)
                    assert ks == max_taps(ext, out, interp)
                    txt = subprocess.run([exe, str(int(interp == "bicubic")), str(ext), str(out), str(ks + 3)], check=True,
                                         capture_output=True, text=True).stdout
                    got = np.array([[int(v) for v in line.split()] for line in txt.strip().split("\n")])
                    ok = np.array_equal(got[:, :2], hb) and np.array_equal(got[:, 2:2 + ks], hk) and not got[:, 2 + ks:].any()
                    n += 1
                    if not ok:
                        bad += 1
                        print("MISMATCH", interp, ext, "->", out)
    print(f"{n} plans compared, {bad} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
