"""The owner gate and the compute-unit lease of SLIM-BPR (csrc/slim_gate.h) on the CPU.

tests/slim_gate_main.cpp is a stand-alone program around the header, built with g++ -fsanitize=address,undefined and run as a child
process, one role per run; a second process is the same program started again.  The lock directory is a temporary one
(MI355REC_LOCK_DIR).  A sanitizer report makes the role's exit status non-zero, which every test checks.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "slim_gate_main.cpp")
LOCK_NAME = "mi355rec_slim_owners_%d_0000_c1_00_0.lock" % os.getuid()          # per user, per bus id (the program's: 0000:c1:00.0)
KNOB_NAMES = ("MI355REC_LOCK_DIR", "XDG_RUNTIME_DIR", "MI355REC_SLIM_NO_OWNER_GATE", "MI355REC_SLIM_GATE_WAIT_S")


def build(out, sanitize, runtimes):
    """(the sanitizer's runtime is linked into the program, so that it does not depend on the order the loader finds libraries in)"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=" + sanitize, "-fno-omit-frame-pointer", "-pthread", SOURCE, "-o", str(out)]
    return subprocess.run(cmd + ["-static-lib" + r for r in runtimes], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slim_gate") / "slim_gate_main"
    done = build(exe, "address,undefined", ("asan", "ubsan"))
    assert done.returncode == 0, done.stderr
    return str(exe)


def environment(lock_dir, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOB_NAMES}
    env["MI355REC_LOCK_DIR"] = str(lock_dir)
    env["UBSAN_OPTIONS"] = "halt_on_error=1"
    env.update(knobs)
    return env


def run_role(program, role, env):
    done = subprocess.run([program, role], env=env, capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, (role, done.stdout, done.stderr)
    return done.stdout.split("\n")[:-1]


class Player:
    """a role that is talked to over its stdin and stdout, a line each"""

    def __init__(self, program, role, env):
        self.p = subprocess.Popen([program, role], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

    def hear(self):
        return self.p.stdout.readline().rstrip("\n")

    def say(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()

    def end(self):
        out, err = self.p.communicate(timeout=60)
        assert self.p.returncode == 0, (out, err)
        return out.split("\n")[:-1]


def test_nested_holders_share_one_file_lock(program, tmp_path):
    assert run_role(program, "nesting", environment(tmp_path))[-1] == "ok"
    assert os.listdir(tmp_path) == [LOCK_NAME]
    assert os.stat(tmp_path / LOCK_NAME).st_mode & 0o777 == 0o600


def test_a_second_process_is_refused_while_the_first_holds(program, tmp_path):
    env = environment(tmp_path)
    assert run_role(program, "probe", env) == ["granted"]
    holder = Player(program, "hold", env)
    assert holder.hear() == "held"
    assert run_role(program, "probe", env) == ["denied"]
    holder.say("release")
    assert holder.hear() == "released"
    assert run_role(program, "probe", env) == ["granted"]               # after the first releases ...
    holder.say("exit")
    holder.end()
    holder = Player(program, "hold", env)
    assert holder.hear() == "held"
    assert run_role(program, "probe", env) == ["denied"]
    holder.say("exit")                                                  # ... or exits with the gate held
    holder.end()
    assert run_role(program, "probe", env) == ["granted"]


def test_no_owner_gate_always_grants_and_creates_no_file(program, tmp_path):
    env = environment(tmp_path, MI355REC_SLIM_NO_OWNER_GATE="1")
    holder = Player(program, "hold", env)
    assert holder.hear() == "held"
    assert run_role(program, "no_gate", env)[-1] == "ok"                # ... while another process "holds"
    holder.say("exit")
    holder.end()
    assert os.listdir(tmp_path) == []


def test_a_symbolic_link_in_the_lock_files_place_is_refused(program, tmp_path):
    lock_dir = tmp_path / "locks"
    lock_dir.mkdir()
    target = tmp_path / "somebody_elses_file"
    target.write_text("precious")
    os.symlink(target, lock_dir / LOCK_NAME)
    env = environment(lock_dir)
    assert run_role(program, "probe", env) == ["denied"]
    assert run_role(program, "no_lock_file", env)[-1] == "ok"
    assert target.read_text() == "precious" and os.path.islink(lock_dir / LOCK_NAME)


def test_without_a_lock_file_the_blocking_gate_serialises_inside_the_process(program, tmp_path):
    assert run_role(program, "no_lock_file", environment(tmp_path / "no_such_directory"))[-1] == "ok"
    assert os.listdir(tmp_path) == []


def test_the_blocking_gate_reports_a_timeout_and_works_afterwards(program, tmp_path):
    env = environment(tmp_path)
    holder = Player(program, "hold", env)
    assert holder.hear() == "held"
    waiter = Player(program, "blocking", environment(tmp_path, MI355REC_SLIM_GATE_WAIT_S="0.2"))
    assert waiter.hear() == "timeout 0.200"
    assert waiter.hear() == "serial free"
    holder.say("exit")
    holder.end()
    waiter.say("go on")
    assert waiter.hear() == "held"
    assert waiter.end()[-1] == "ok"


def test_two_threads_take_turns(program, tmp_path):
    assert run_role(program, "threads", environment(tmp_path))[-1] == "ok"


def test_two_threads_take_turns_under_the_thread_sanitizer(tmp_path):
    exe = tmp_path / "slim_gate_main_tsan"
    done = build(exe, "thread", ("tsan",))
    if done.returncode != 0 and ("tsan" in done.stderr or "-fsanitize=thread" in done.stderr):
        pytest.skip("no ThreadSanitizer runtime for g++ on this machine")
    assert done.returncode == 0, done.stderr
    (tmp_path / "locks").mkdir()
    assert run_role(str(exe), "threads", environment(tmp_path / "locks"))[-1] == "ok"


def test_lease_arithmetic_at_256_compute_units(program, tmp_path):
    assert run_role(program, "lease", environment(tmp_path))[-1] == "ok"
