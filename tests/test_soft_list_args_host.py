"""CPU: the soft light list's argument rule (rts_args.h: softListOk, shared by the library and the host twin) in a host program of its
own under the address and undefined-behaviour sanitizers -- nothing sanitized is loaded into Python."""
import os
import subprocess


def test_soft_list_argument_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/soft_list_args_host.cpp, -fsanitize=address,undefined: softListOk over every (type 0..2, nsamples 0..50, first 0..50)
    in the first entry, the last entry and an entry beyond the count of lists of 1, 3 and 8 lights, every count 0..10, radii of every
    class, NULL, and values at the ends of uint32, against a restatement of include/rts.h written the slow way."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "soft_list_args_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(root, "tests", "cpp", "soft_list_args_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 3 * 51 * 51 * 7, run.stdout[-2000:]
