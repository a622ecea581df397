"""CPU: the guard every soft light list launcher applies to its argument block's 64 x 4 floats (rts_soft_list_slots.h: softListSlotsOk)
in a host program of its own under the address and undefined-behaviour sanitizers -- nothing sanitized is loaded into Python."""
import os
import subprocess


def test_soft_list_slot_guard_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/soft_list_slots_host.cpp, -fsanitize=address,undefined: over the grid of soft_list_tables_host.cpp and probes at the
    ends of their range, the slots the header's own writers write for a list are accepted exactly where softListTablesOk accepts the
    list; a slot with type 2, samples 0 or 49, first + samples = 49, k = samples or first + T = 49 is refused."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "soft_list_slots_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(root, "tests", "cpp", "soft_list_slots_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100000, run.stdout[-2000:]
