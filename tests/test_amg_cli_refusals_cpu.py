"""CPU: what the pemspgemm CLI refuses of `--solve cg|bicgstab --amg smoothed|plain` before it opens a device: one line and exit
code 1 each, in the style of test_krylov_cli_refusals_cpu.py."""
import importlib
import subprocess


def test_amg_refusals(pkg, tmp_path):
    hostio = importlib.import_module("pem_spgemm_amd.hostio")
    fa = tmp_path / "A.mtx"
    fa.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n2 2 2.0\n")
    fb = tmp_path / "b.mtx"
    fb.write_text("%%MatrixMarket matrix array real general\n2 1\n1\n2\n")
    b = ["--rhs", str(fb)]
    for args, line in ((["--amg", "smoothed"], "--amg needs --solve cg|bicgstab. Exiting."),
                       (["--amg", "nonsense"], "--amg needs --solve cg|bicgstab. Exiting."),
                       (["--solve", "cg", "--amg", "smoothed", "--precond", "jacobi"] + b, "--amg does not combine with --precond. Exiting."),
                       (["--solve", "bicgstab", "--amg", "plain", "--precond", "none"] + b, "--amg does not combine with --precond. Exiting."),
                       (["--solve", "cg", "--amg", "sa"] + b, "--amg sa: unknown kind (smoothed, plain). Exiting."),
                       (["--solve", "bicgstab", "--amg", "Smoothed"] + b, "--amg Smoothed: unknown kind (smoothed, plain). Exiting."),
                       # the lines that stay as they are
                       (["--solve", "cg", "--amg", "smoothed"], "--solve cg needs --rhs b.mtx. Exiting."),
                       (["--solve", "cg", "--precond", "amg"] + b, "--precond amg: unknown preconditioner (none, jacobi, ilu0). Exiting."),
                       (["--solve", "cg", "--amg", "plain", "--gpus", "2"] + b, "--solve does not combine with --gpus. Exiting.")):
        out = subprocess.run([hostio.CLI_PATH, str(fa), "0", *args], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert out.returncode == 1, (args, out.stdout, out.stderr)
        assert out.stdout.strip().splitlines()[-1] == line, (args, out.stdout)
