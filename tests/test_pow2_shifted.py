"""csrc/ntt_shift.h: the 16-point transform at shifted points (ntt_pow2_points_shifted) that k_lde_pass2_fused uses for the
power-of-two part of its coset scale.  tests/pow2_shifted_dump.cpp (g++, host only: ntt_shift.h and what it includes) compares it
with the plain transform of the inputs multiplied by 2^(S brev4(e)), for every shift the kernel instantiates, on the words at the
edges of the carry chains (0, 1, p - 1, 2^32 - 1, 2^32, p - 2^32 in every position) and on random words."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SHIFTS = (0, 39, 78, 117)   # csrc/ntt.hip, k_lde_pass2_fused: 2^(39 kappa), 2^(78 kappa)


def test_shifted_transform_is_the_plain_transform_of_scaled_inputs(tmp_path):
    exe = str(tmp_path / "pow2_shifted_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-Wno-unused-parameter",
                           "-DTVM_EMU", "-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "triton_vm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "pow2_shifted_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], text=True, stdout=subprocess.PIPE)
    print(run.stdout)
    lines = {int(w[1]): (int(w[3]), int(w[5])) for w in (line.split() for line in run.stdout.splitlines())}
    assert run.returncode == 0, run.stdout
    for shift in KERNEL_SHIFTS:
        cases, mismatches = lines[shift]
        assert cases > 2000 and mismatches == 0, (shift, cases, mismatches)
