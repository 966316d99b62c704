"""CPU: what the pemspgemm CLI refuses of `--solve cg|bicgstab --rhs b.mtx [--precond ..] [--rtol R] [--max-iters N]` before it opens a
device: one line and exit code 1 each, in the style of test_cli_refusals_cpu.py."""
import importlib
import subprocess


def test_solve_refusals(pkg, tmp_path):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    fb = tmp_path / "b.mtx"
    fb.write_text("%%MatrixMarket matrix array real general\n2 1\n1\n2\n")
    fb2 = tmp_path / "b2.mtx"
    fb2.write_text("%%MatrixMarket matrix array real general\n2 2\n1\n2\n3\n4\n")
    b = ["--rhs", str(fb)]
    for args, line in ((["--solve", "cg", "--gpus", "2"] + b, "--solve does not combine with --gpus. Exiting."),
                       (["--solve", "bicgstab", "--power", "2"] + b, "--solve does not combine with --power. Exiting."),
                       (["--solve", "cg", "--trsv", "lower"] + b, "--solve does not combine with --trsv. Exiting."),
                       (["--solve", "cg", "--reduce", "rows"] + b, "--solve does not combine with --reduce. Exiting."),
                       (["--solve", "cg", "--components"] + b, "--solve does not combine with --components. Exiting."),
                       (["--solve", "cg"], "--solve cg needs --rhs b.mtx. Exiting."),
                       (["--solve", "gmres"] + b, "--solve gmres: unknown method (cg, bicgstab). Exiting."),
                       (["--solve", "cg", "--precond", "ssor"] + b, "--precond ssor: unknown preconditioner (none, jacobi, ilu0). Exiting."),
                       (["--solve", "cg", "--rtol", "-1"] + b, "--rtol -1: want a number >= 0. Exiting."),
                       (["--solve", "cg", "--rtol", "tiny"] + b, "--rtol tiny: want a number >= 0. Exiting."),
                       (["--solve", "cg", "--rtol", "nan"] + b, "--rtol nan: want a number >= 0. Exiting."),
                       (["--solve", "cg", "--max-iters", "-3"] + b, "--max-iters -3: want an integer >= 0. Exiting."),
                       (["--solve", "cg", "--max-iters", "1.5"] + b, "--max-iters 1.5: want an integer >= 0. Exiting."),
                       (["--precond", "jacobi"], "--precond / --rtol / --max-iters need --solve cg|bicgstab. Exiting."),
                       (["--rtol", "1e-6"], "--precond / --rtol / --max-iters need --solve cg|bicgstab. Exiting."),
                       (["--rhs", str(fb)], "--rhs needs --trsv lower|upper[:unit]. Exiting."),
                       (["--solve", "cg", "--rhs", str(fb2)], f"--rhs {fb2}: an array of 2 columns, not of one. Exiting."),
                       (["--solve", "cg", "--rhs", str(tmp_path / "none.mtx")],
                        f"--rhs {tmp_path / 'none.mtx'}: cannot open the file (want a Matrix-Market array real general file). Exiting."),
                       (["--sampled", str(fa), "--solve", "cg"] + b, None)):
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1, (args, out.stdout, out.stderr)
        if line is None:
            assert "does not combine with --solve" in out.stdout, out.stdout
        else:
            assert out.stdout.strip().splitlines()[-1] == line, (args, out.stdout)
