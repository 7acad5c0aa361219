"""The decoder-form rule with the soft multi-lane switch (decoder_form.hpp: FormKnobs::soft_lanes and the two soft knobs): a stand-alone program,
tests/host_sanitize/soft_forms_unit.cpp, compiled with g++ -fsanitize=address,undefined and run, the way test_host_sanitize.py runs host_units.cpp.
CPU build only; the rule makes no GPU call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "host_sanitize")


def test_soft_form_rule_under_sanitizer():
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    exe = os.path.join(HERE, "build", "soft_forms_unit_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(HERE, "soft_forms_unit.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("DABHIP_SOFT_LANES", "DABHIP_VIT_SOFT_FOUR_LANES", "DABHIP_FIC_SOFT_FOUR_LANES"):
        env.pop(name, None)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert run.stdout.split() == ["ok", "soft-forms"]
