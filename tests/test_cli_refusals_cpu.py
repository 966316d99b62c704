"""CPU: every command line the pemspgemm CLI refuses before it opens a device gets, byte for byte, the message and the exit code
recorded in tests/golden/cli_refusals.json (tests/golden/make_cli_refusals.py: recorded with the binary of the commit before main()
was split into stages).  The records cover each "needs", each unknown name, the bad thunks and sources, each pair that does not
combine, each error of the two Matrix-Market array readers, and command lines with two or three faults -- which pin the order of
the checks."""
import importlib
import json
import os
import subprocess

import pytest

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals.json")) as _f:
    RECORDS = json.load(_f)


def test_records_cover_the_refusals():
    text = "".join(r["stdout"] for r in RECORDS)
    for word in ("Provide a matrix market file path", "--mask-complement needs", "--alpha / --beta need --add", "--assign-rows needs", "--assign-cols needs",
                 "--assign-accum needs", "--sddmm-y needs", "unknown semiring", "unknown op upper", "unknown dimension", "unknown op avg",
                 "--assign-accum avg: unknown op", "does not parse as a number", "needs an integral thunk", "want a 1-based vertex number",
                 "K must be at least 2", "need the plus_times semiring", "--gpus does not combine with --fp32 / --cache",
                 "cannot open the file", "empty file", "no Matrix-Market header", "not an array (dense) file", "not a real one",
                 "not an integer or real one", "not a general one", "no size line", "bad size line", "fewer values than rows x cols",
                 "fewer values than the size line says", "is not an integer", "is out of range", "a list of 0 indices", "is repeated", "an array of 2 columns",
                 "Y has 2 columns, X has 1"):
        assert word in text, word
    one_device = ["--gpus", "--power"]
    clashes = {"--power": ["--gpus", "--mask", "--B", "the A*A^T argument"], "--add": ["--gpus", "--mask", "--power"], "--select": one_device,
               "--extract-rows": one_device, "--extract-cols": one_device, "--assign-into": one_device, "--reduce": one_device,
               "--spmm": one_device + ["--reduce"], "--sddmm": one_device + ["--reduce", "--spmm"],
               "--bfs": one_device + ["--reduce", "--spmm", "--sddmm"], "--gpus": ["--semiring min_plus", "--mask", "--fp32 / --cache"]}
    for flag, others in clashes.items():
        for other in others:
            assert f"{flag} does not combine with {other}" in text, (flag, other)
    assert all(r["returncode"] == 1 for r in RECORDS)


@pytest.mark.parametrize("k", range(len(RECORDS)), ids=[f"{k:03d}" + "".join(a for a in r["args"] if a.startswith("--")) for k, r in enumerate(RECORDS)])
def test_refusal(k, pkg, tmp_path):
    rec = RECORDS[k]
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    for name, text in rec["files"].items():
        (tmp_path / name).write_text(text)
    args = [a.replace("{tmp}", str(tmp_path)) for a in rec["args"]]
    out = subprocess.run([hostio.CLI_PATH, *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.stdout.replace(str(tmp_path), "{tmp}") == rec["stdout"]
    assert out.returncode == rec["returncode"], out.stderr
