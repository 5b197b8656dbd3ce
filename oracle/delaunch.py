"""delaunch.py IN OUT - rewrites every kernel launch statement `name<<<grid, block>>>(` of the C++ text IN to
`PTMI_REF_LAUNCH(name, grid, block)(` and writes the result to OUT, so that a host compiler can parse it.

TEST INFRASTRUCTURE ONLY (oracle/Makefile, _ref/libptmi_ref_solver.so).  OUT must lie outside the repository: the recipe
gives a temporary directory and removes it when it ends.  The filter fails (exit status 1, nothing written) unless
  - it replaced exactly the launch sites it found: as many as there are `<<<` and as there are `>>>` in IN, at least one;
  - the text outside the replaced spans is unchanged, and the text inside them kept the kernel's name and both launch
    arguments, character for character.
"""
import os
import re
import sys

LAUNCH = re.compile(r"([A-Za-z_]\w*)(\s*)<<<([^<>;]*?)>>>(\s*)\(")


def delaunch(text):
    out, outside_in, outside_out, last, sites = [], [], [], 0, 0
    for m in LAUNCH.finditer(text):
        name, _, args, _ = m.groups()
        if args.count(",") != 1:
            raise ValueError(f"launch of {name}: expected <<<grid, block>>>, found <<<{args}>>>")
        out.append(text[last:m.start()]); outside_in.append(text[last:m.start()])
        out.append(f"PTMI_REF_LAUNCH({name}, {args.strip()})(")
        last = m.end(); sites += 1
    out.append(text[last:]); outside_in.append(text[last:])
    new = "".join(out)
    if sites == 0 or sites != text.count("<<<") or sites != text.count(">>>"):
        raise ValueError(f"{sites} launch statements rewritten, but the text holds {text.count('<<<')} '<<<' and {text.count('>>>')} '>>>'")
    if "<<<" in new or ">>>" in new:
        raise ValueError("a launch bracket survived the rewrite")
    # second, independent pass over the OUTPUT: take the replacements out again and compare what is left with the input's
    back = re.compile(r"PTMI_REF_LAUNCH\(([A-Za-z_]\w*), ([^()]*?)\)\(")
    last = 0
    found = []
    for m in back.finditer(new):
        outside_out.append(new[last:m.start()]); last = m.end(); found.append((m.group(1), m.group(2)))
    outside_out.append(new[last:])
    if outside_out != outside_in:
        raise ValueError("the text outside the rewritten launch statements changed")
    want = [(m.group(1), m.group(3).strip()) for m in LAUNCH.finditer(text)]
    if found != want:
        raise ValueError("a rewritten launch statement lost its kernel name or its launch arguments")
    return new, sites


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr); return 2
    src, dst = argv[1], argv[2]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.commonpath([repo, os.path.abspath(dst)]) == repo:
        print(f"delaunch: {dst} lies inside the repository", file=sys.stderr); return 1
    with open(src, encoding="utf-8") as f:
        text = f.read()
    try:
        new, sites = delaunch(text)
    except ValueError as e:
        print(f"delaunch: {src}: {e}", file=sys.stderr); return 1
    with open(dst, "w", encoding="utf-8") as f:
        f.write(new)
    print(f"[oracle] delaunch: {sites} launch statements rewritten")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
