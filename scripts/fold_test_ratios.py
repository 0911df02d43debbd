#!/usr/bin/env python3
"""Fold the per-case figures that tests/test_mlp_kernels.py prints under `pytest -s` into one table: per entry (mlp2, parts, tail)
and tensor kind the range of `ours / literal` with the case of its largest value, then the largest ratio among the figures whose
error lies above the 2^-20 floor (where the factor 4 carries the bound).  Reads the saved output of

    python -m pytest tests/test_mlp_abi.py tests/test_mlp_kernels.py -m "not gpu" -s -q     (or -m gpu)

    python scripts/fold_test_ratios.py pytest_output.txt

This is how the tables at the head of profiles/mlp_kernels/*_tests_tail.txt and the ranges in the test's docstring were made."""
import collections
import re
import sys

FLOOR = 2.0 ** -20


def main(path):
    ratios = collections.defaultdict(list)
    above, worst = 0, (0.0, None)
    for line in open(path):
        line = line.strip().lstrip(".")
        m = re.match(r"^(.*) (\w+): ours / literal ([\d.]+|inf|nan)$", line)
        if m:
            what, kind, v = m.groups()
            ratios[("parts" if what.startswith("mlp2 parts") else what.split()[0], kind)].append((float(v), what))
        m = re.match(r"^(.*) (\w+): err (\S+) gap (\S+) bound (\S+)$", line)
        if m:
            what, kind, err, gap = m.group(1), m.group(2), float(m.group(3)), float(m.group(4))
            if err > FLOOR:
                above += 1
                if gap > 0 and err / gap > worst[0]:
                    worst = (err / gap, f"{kind} {what} err {err:.3e} gap {gap:.3e}")
    for (entry, kind), vs in sorted(ratios.items()):
        vs.sort()
        print(f"{entry:6s} {kind:7s} n={len(vs):4d} {vs[0][0]:.2f} - {vs[-1][0]:.2f}   max at: {vs[-1][1]}")
    print(f"{above} figures above the floor; largest ratio among them: {worst[0]:.2f} ({worst[1]})")


if __name__ == "__main__":
    main(sys.argv[1])
