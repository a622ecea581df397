"""CPU: the adaptive trace's argument rule (rts_args.h: adaptiveLightOk, shared by the library and the host twin) in a host program of
its own under the address and undefined-behaviour sanitizers -- nothing sanitized is loaded into Python."""
import os
import subprocess


def test_adaptive_argument_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/adaptive_args_host.cpp, -fsanitize=address,undefined: adaptiveLightOk over every (type 0..2, nsamples 0..66,
    table 0..66, probe 0..66), NULL, and values at the ends of uint32, against a restatement of include/rts.h written the slow way."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "adaptive_args_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(root, "tests", "cpp", "adaptive_args_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 3 * 67 * 67 * 67, run.stdout[-2000:]
