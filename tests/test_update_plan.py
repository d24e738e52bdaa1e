"""The plan of a scene update (csrc/host/update_plan.h plan_update: which parts of lumc_scene_update run, from the caller's dirty flags and the context's modes), no GPU.

tests/support/update_plan_check.cpp holds every field of the plan, update_counts_and_tables' two conditions and the plan after a fallback from the in-place path to
the flag statements scene_update consisted of before the plan, transcribed there word for word, for all 1024 x 2 x 2 x 2 x 2 inputs."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_input_gives_the_plan_the_flag_statements_gave(tmp_path):
    exe = str(tmp_path / "update_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "support", "update_plan_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)  # (the runtimes are linked statically: the program needs nothing preloaded)
    print(ran.stdout[-400:])
    assert ran.returncode == 0 and "update_plan_check: 16384 of 16384 cases agree" in ran.stdout and "update_plan_check: ok" in ran.stdout, ran.stdout[-4000:]
