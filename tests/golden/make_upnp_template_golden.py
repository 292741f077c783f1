"""Digests of the reference's 141 x 149 UPnP elimination template (sfm/pose/build_upnp_action_matrix_using_symmetry.cc), for
tests/test_upnp.py::test_template_layout_reproduces_the_reference_assignments, written to tests/golden/upnp_template_digest.json.

Three sets are read from the reference's text, each reduced to a count and the sha256 of a canonical listing (data, not source
text: none of the statements can be recovered from a digest):
  * template : the (row, column, equation, input column) quadruples of SetUpTemplateMatrixUsingSymmetry's M2(r, c) = M1(i, j);
  * input    : the terms (coefficient, A row, A column) / (coefficient, b index) of the input matrix' cost-derivative rows
               M1(i < 4, j), in the reference's order;
  * fixed    : the constant entries M1(4 .. 7, j) = +-1 of the rows q_i (|q|^2 - 1).
The test rebuilds the same three sets from the committed layout header and from the rule of scripts/gen_upnp_layout.py and
compares the digests, so it needs no copy of the reference.

  python tests/golden/make_upnp_template_golden.py <reference source root>"""
import hashlib
import json
import os
import re
import sys

SRC_REL = os.path.join("src", "theia", "sfm", "pose", "build_upnp_action_matrix_using_symmetry.cc")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "upnp_template_digest.json")


def digest(items):
    """count and sha256 of a set / list of integer tuples (sorted, one tuple per line)"""
    lines = sorted(repr(tuple(t)) for t in items)
    return len(lines), hashlib.sha256("\n".join(lines).encode()).hexdigest()


def parse_reference(text):
    setup = text[text.index("void SetUpTemplateMatrixUsingSymmetry"):text.index("Matrix8d BuildActionMatrixUsingSymmetry")]
    template = [tuple(int(v) for v in m) for m in re.findall(r"M2\((\d+), (\d+)\) = M1\((\d+), (\d+)\);", setup)]
    body = text[text.index("Matrix8d BuildActionMatrixUsingSymmetry"):]
    inp = []
    for mm in re.finditer(r"M1\((\d), (\d+)\) = ([^;]*);", body):
        i, j, rhs = int(mm.group(1)), int(mm.group(2)), mm.group(3)
        if i >= 4:
            continue
        got = tuple((int(c), int(a), int(b)) for c, a, b in re.findall(r"(\d) \* M\((\d+), (\d+)\)", rhs))
        lin = tuple((int(c), int(k)) for c, k in re.findall(r"(\d) \* C\[(\d+)\]", rhs))
        inp.append((i, j, got, lin))
    fixed = [(int(a), int(b), int(v)) for a, b, v in re.findall(r"M1\(([4-7]), (\d+)\) = (-?1);", body)]
    return template, inp, fixed


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    text = open(os.path.join(sys.argv[1], SRC_REL)).read()
    template, inp, fixed = parse_reference(text)
    out = {"source": "sfm/pose/build_upnp_action_matrix_using_symmetry.cc (SetUpTemplateMatrixUsingSymmetry, BuildActionMatrixUsingSymmetry)"}
    for name, items in (("template", template), ("input", inp), ("fixed", fixed)):
        n, h = digest(items)
        out[name] = {"count": n, "sha256": h}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote %s: %s" % (os.path.basename(OUT), {k: v["count"] for k, v in out.items() if k != "source"}))


if __name__ == "__main__":
    main()
