"""lookupPaths of the JNI glue (jni/deltareplay_jni.c) on the mock JNIEnv, as its own sanitized
program (tests/native/jni_mock_lookup.c): arrays and lengths reach dr_state_lookup_paths as given and
the results reach the Java arrays; a null array, an empty pathOff, outputs shorter than the paths
and offsets beyond pathBytes raise IllegalArgumentException before the library is called; a library
error keeps its exception class and message and leaves the outputs alone; an array the JVM cannot
hand out ends the call; every array handed out is handed back on every path, and no scenario makes
a JNI call while an exception is pending."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLUE = os.path.join(ROOT, "jni", "deltareplay_jni.c")
MOCK = os.path.join(ROOT, "tests", "native", "jni_mock_lookup.c")
SCENARIOS = ["lookup_pass_through", "lookup_longer_outputs", "lookup_no_paths", "lookup_null_arrays",
             "lookup_lengths_refused", "lookup_offsets_beyond_bytes", "lookup_library_error",
             "lookup_array_failure_releases"]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_lookup_paths_on_a_mock_jni_env(tmp_path):
    mock_src = open(MOCK).read()
    defined = set(re.findall(r"^\S[^(\n]*\b(dr_\w+)\(", mock_src, re.M))
    assert "dr_state_lookup_paths" in defined
    called = set(re.findall(r"\b(dr_\w+)\(", open(GLUE).read()))
    assert "dr_state_lookup_paths" in called
    gen = tmp_path / "gen_stubs.c"
    gen.write_text("".join("int %s() { return 15; }\n" % f for f in sorted(called - defined)))
    exe = tmp_path / "jni_mock_lookup"
    inc = ["-I", os.path.join(ROOT, "tests", "native", "jni_min"), "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "native")]
    r = subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-Wno-builtin-declaration-mismatch"] + inc + [GLUE, MOCK, str(gen), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines == [s + " ok" for s in SCENARIOS], run.stdout + run.stderr


def test_lookup_paths_is_bound_in_scala():
    scala = open(os.path.join(ROOT, "jni", "DeltaReplayNative.scala")).read()
    assert re.search(r"@native def lookupPaths\(state: Long, pathBytes: Array\[Byte\], pathOff: Array\[Long\], "
                     r"hitOut: Array\[Byte\], rowOut: Array\[Long\]\): Unit", scala)
