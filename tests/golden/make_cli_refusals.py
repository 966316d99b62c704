#!/usr/bin/env python3
"""Records what the pemspgemm CLI prints when it refuses a command line before it opens a device: cli_refusals.json.

    make_cli_refusals.py <path to a pemspgemm binary>

The binary is the one of the commit BEFORE a change to the CLI's source (built in a scratch worktree of that commit), never the
changed one: tests/test_cli_refusals_cpu.py then holds the changed CLI to the old wording, exit code and -- where a command line
has two or three faults -- to the old choice of which one is reported.  The file committed here was recorded with the binary of
the commit that precedes the split of main() into stages.

Every record is {args, files, returncode, stdout}.  `{tmp}` in args and stdout stands for the directory the files (name ->
content) are written to; no record needs a matrix file, because every refusal here comes before the matrix is read.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
A = "{tmp}/A.mtx"   # never read: the refusals come first

HEAD = "%%MatrixMarket matrix array {} general\n"
FILES = {
    # good ones
    "list.mtx": HEAD.format("integer") + "2 1\n1\n2\n",
    "x.mtx": HEAD.format("real") + "2 1\n1.0\n2.0\n",
    "y2.mtx": HEAD.format("real") + "2 2\n1.0\n2.0\n3.0\n4.0\n",
    # one fault each
    "empty.mtx": "",
    "noheader.mtx": "1 1\n1\n",
    "banner.mtx": "%%MatrixMarkt matrix array real general\n1 1\n1\n",
    "coord.mtx": "%%MatrixMarket matrix coordinate real general\n1 1 1\n1 1 1.0\n",
    "complex.mtx": HEAD.format("complex") + "1 1\n1.0 0.0\n",
    "integer.mtx": HEAD.format("integer") + "1 1\n1\n",
    "symmetric.mtx": "%%MatrixMarket matrix array real symmetric\n1 1\n1.0\n",
    "nosize.mtx": HEAD.format("real") + "% only a comment\n",
    "badsize.mtx": HEAD.format("real") + "x y\n1\n",
    "few.mtx": HEAD.format("real") + "2 1\n1\n",
    "fraction.mtx": HEAD.format("real") + "2 1\n1.5\n2\n",
    "zero.mtx": HEAD.format("integer") + "2 1\n0\n1\n",
    "nolist.mtx": HEAD.format("integer") + "0 1\n",
    "repeat.mtx": HEAD.format("integer") + "2 1\n1\n1\n",
    "twocols.mtx": HEAD.format("integer") + "2 2\n1\n2\n1\n2\n",
}


def t(name):
    return "{tmp}/" + name


def vectors():
    v = [[]]                                                           # no argument at all
    v += [[A, "0", "x", "y"], ["--standin", "scircuit", "0", "x", "y"], [A, "0", "x", "--B"]]   # too many positional arguments
    # "needs"
    v += [[A, "--mask-complement"], [A, "--alpha", "2"], [A, "--beta", "0.5"], [A, "--assign-rows", t("list.mtx")],
          [A, "--assign-cols", t("list.mtx")], [A, "--assign-accum", "plus"], [A, "--sddmm-y", t("x.mtx")]]
    # unknown names
    v += [[A, "--semiring", "plus_min"], [A, "--select", "upper"], [A, "--select", "upper:3"], [A, "--reduce", "diag"],
          [A, "--reduce", "rows:avg"], [A, "--assign-into", A, "--assign-accum", "avg"]]
    # thunks, sources, powers
    v += [[A, "--select", "value_gt:abc"], [A, "--select", "value_gt:"], [A, "--select", "value_gt:1x"], [A, "--select", "tril:0.5"],
          [A, "--select", "col_gt:1e10"], [A, "--bfs", "0"], [A, "--bfs", "x"], [A, "--bfs", "3x"], [A, "--bfs", "-2"],
          [A, "--power", "1"], [A, "--power", "-3"]]
    # --add with a scale under a semiring that has no scaling
    v += [[A, "--add", A, "--alpha", "2", "--semiring", "min_plus"], [A, "--add", A, "--beta", "2", "--semiring", "lor_land"]]
    # every "does not combine with" pair of the source
    v += [[A, "--power", "2", "--gpus", "2"], [A, "--power", "2", "--mask", A], [A, "--power", "2", "--B", A], [A, "0", "1", "--power", "2"],
          [A, "--add", A, "--gpus", "2"], [A, "--add", A, "--mask", A], [A, "--add", A, "--power", "2"],
          [A, "--select", "tril", "--gpus", "2"], [A, "--select", "tril", "--power", "2"],
          [A, "--extract-rows", t("list.mtx"), "--gpus", "2"], [A, "--extract-rows", t("list.mtx"), "--power", "2"],
          [A, "--extract-cols", t("list.mtx"), "--gpus", "2"], [A, "--extract-cols", t("list.mtx"), "--power", "2"],
          [A, "--assign-into", A, "--gpus", "2"], [A, "--assign-into", A, "--power", "2"],
          [A, "--spmm", t("x.mtx"), "--gpus", "2"], [A, "--spmm", t("x.mtx"), "--power", "2"], [A, "--spmm", t("x.mtx"), "--reduce", "rows"],
          [A, "--sddmm", t("x.mtx"), "--gpus", "2"], [A, "--sddmm", t("x.mtx"), "--power", "2"], [A, "--sddmm", t("x.mtx"), "--reduce", "cols"],
          [A, "--sddmm", t("x.mtx"), "--spmm", t("x.mtx")],
          [A, "--reduce", "rows", "--gpus", "2"], [A, "--reduce", "rows", "--power", "2"],
          [A, "--bfs", "1", "--gpus", "2"], [A, "--bfs", "1", "--power", "2"], [A, "--bfs", "1", "--reduce", "rows"],
          [A, "--bfs", "1", "--spmm", t("x.mtx")], [A, "--bfs", "1", "--sddmm", t("x.mtx")],
          [A, "--gpus", "2", "--semiring", "min_plus"], [A, "--gpus", "2", "--mask", A], [A, "--gpus", "2", "--fp32"],
          [A, "--gpus", "2", "--cache", "{tmp}"]]
    # two or three faults at once: which message wins
    v += [[A, "--spmm", t("x.mtx"), "--reduce", "rows", "--gpus", "2"],
          [A, "--power", "2", "--B", A, "--mask", A],
          [A, "--extract-rows", t("fraction.mtx"), "--assign-into", A, "--assign-accum", "avg"],
          [A, "--mask-complement", "--semiring", "plus_min"],
          [A, "--semiring", "plus_min", "--power", "1"],
          [A, "--power", "1", "--gpus", "2"],
          [A, "--alpha", "2", "--select", "upper"],
          [A, "--bfs", "0", "--reduce", "rows"],
          [A, "--sddmm-y", t("x.mtx"), "--spmm", t("missing.mtx")],
          [A, "--select", "tril:x", "--extract-rows", t("missing.mtx"), "--bfs", "x"],
          [A, "--gpus", "2", "--fp32", "--mask", A],
          [A, "--reduce", "diag:avg", "--bfs", "0"],
          [A, "--assign-rows", t("list.mtx"), "--assign-accum", "plus", "--sddmm-y", t("x.mtx")],
          [A, "--add", A, "--alpha", "2", "--semiring", "min_plus", "--select", "upper"],
          [A, "0", "x", "y", "--mask-complement"],
          [A, "--assign-into", A, "--assign-accum", "avg", "--assign-rows", t("missing.mtx")],
          [A, "--assign-into", A, "--assign-rows", t("repeat.mtx"), "--assign-cols", t("zero.mtx"), "--reduce", "diag"],
          [A, "--sddmm", t("x.mtx"), "--sddmm-y", t("y2.mtx"), "--bfs", "x"],
          [A, "--extract-cols", t("zero.mtx"), "--extract-rows", t("twocols.mtx")],
          [A, "--gpus", "2", "--semiring", "min_plus", "--power", "1"],
          [A, "--select", "tril", "--power", "2", "--add", A]]
    # the two array readers: every error string, through every flag that reads such a file
    both = ["missing.mtx", "empty.mtx", "noheader.mtx", "banner.mtx", "coord.mtx", "complex.mtx", "symmetric.mtx", "nosize.mtx", "badsize.mtx", "few.mtx"]
    for name in both + ["integer.mtx"]:
        v.append([A, "--spmm", t(name)])
    for name in both + ["fraction.mtx", "zero.mtx", "nolist.mtx", "twocols.mtx"]:
        v.append([A, "--extract-rows", t(name)])
    v += [[A, "--extract-cols", t("few.mtx")], [A, "--sddmm", t("coord.mtx")], [A, "--sddmm", t("x.mtx"), "--sddmm-y", t("few.mtx")],
          [A, "--sddmm", t("x.mtx"), "--sddmm-y", t("y2.mtx")],
          [A, "--assign-into", A, "--assign-rows", t("repeat.mtx")], [A, "--assign-into", A, "--assign-cols", t("repeat.mtx")],
          [A, "--assign-into", A, "--assign-rows", t("zero.mtx")], [A, "--assign-into", A, "--assign-cols", t("twocols.mtx")]]
    return v


def main():
    cli = os.path.abspath(sys.argv[1])
    records = []
    for args in vectors():
        files = {name: FILES[name] for name in FILES if any(a == t(name) for a in args)}
        with tempfile.TemporaryDirectory() as tmp:
            for name, text in files.items():
                with open(os.path.join(tmp, name), "w") as f:
                    f.write(text)
            out = subprocess.run([cli] + [a.replace("{tmp}", tmp) for a in args], capture_output=True, text=True, timeout=60, cwd=tmp)
            stdout = out.stdout.replace(tmp, "{tmp}")
        assert out.returncode == 1 and stdout.endswith("Exiting.\n") and out.stderr == "", (args, out.returncode, stdout, out.stderr)
        records.append({"args": args, "files": files, "returncode": out.returncode, "stdout": stdout})
    with open(os.path.join(HERE, "cli_refusals.json"), "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    print(len(records), "records written")


if __name__ == "__main__":
    main()
