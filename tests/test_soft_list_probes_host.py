"""CPU: the argument rule of the adaptive soft light list's probe counts (rts_args.h: softListProbesOk, shared by the library and the
host twin) in a host program of its own under the address and undefined-behaviour sanitizers -- nothing sanitized is loaded into
Python."""
import os
import subprocess


def test_soft_list_probes_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/soft_list_probes_host.cpp, -fsanitize=address,undefined: softListProbesOk over every (nsamples 0..50, probe 0..51) in
    the first and the last entry of lists of 1, 3 and 8 lights -- the probes in a heap array of exactly `count` entries --, hard entries,
    lists the list rule refuses, NULL for either argument and values at the ends of uint32, against a restatement of include/rts.h
    written the slow way."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "soft_list_probes_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(root, "tests", "cpp", "soft_list_probes_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 51 * 52 * 5 * 2, run.stdout[-2000:]
