"""Import BEFORE m17hip: the measurement build of the library (make -C m17-cxx-demod_amd/csrc tools -> libm17hip_tools.so: section timers,
per-wave times, schedule experiment knobs) unless M17HIP_LIB names another build.

Also the rank launcher of the multi-GPU tools (`launch_ranks`): a tool that takes the environment of its ranks from a copy made BEFORE this
import (impairment_sweep.py) runs them on the product library."""
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("M17HIP_LIB", os.path.join(ROOT, "m17-cxx-demod_amd", "libm17hip_tools.so"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")


def rank_commands(script, n, argv, port):
    """The N (argv, environment additions) pairs a tool started with --gpus N and no launcher around it starts: one process per GPU,
    rendezvous on 127.0.0.1 — what `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P`
    sets for its workers.  The ranks get the tool's own arguments, without --dry-launch."""
    out = []
    for r in range(n):
        env = {"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n), "GROUP_RANK": "0",
               "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)}
        out.append(([sys.executable, os.path.abspath(script)] + [a for a in argv if a != "--dry-launch"], env))
    return out


def launch_ranks(script, n, argv, result_key, timeout_s, dry_launch=False, base_env=None):
    """Start the N ranks of `script` as child processes (before anything in this process touches the GPU), relay rank 0's JSON result line
    (the line that starts with "{" and holds `result_key`) as the LAST line of stdout; everything else any rank prints goes to stderr, tagged.
    Returns the worst child's exit code.  A failing rank stops the others (they would wait in a collective for ever); after `timeout_s`
    seconds all are stopped (exit code 124); never a retry.  `base_env`: the environment the ranks start from (default: this process's).

    bench.py has the same launcher, but it names its own file and its own result line and bench.py is frozen (it decides how every change
    is measured): the tools get this copy instead of a dependency on bench.py's internals."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmds = rank_commands(script, n, argv, port)
    if dry_launch:
        print(json.dumps({"dry_launch": [{"rank": r, "argv": c, "env": e} for r, (c, e) in enumerate(cmds)]}))
        return 0
    base = dict(os.environ if base_env is None else base_env)
    procs = [subprocess.Popen(c, env={**base, **e}, stdout=subprocess.PIPE, stderr=None, text=True, bufsize=1) for c, e in cmds]
    line0 = []

    def pump(r, pr):
        for ln in pr.stdout:
            s_ = ln.rstrip("\n")
            if r == 0 and s_.startswith("{") and f'"{result_key}"' in s_:
                line0.append(s_)
            else:
                print(f"[rank {r}] {s_}", file=sys.stderr, flush=True)

    threads = [threading.Thread(target=pump, args=(r, pr), daemon=True) for r, pr in enumerate(procs)]
    for t in threads:
        t.start()
    worst, alive, stopped = 0, set(range(n)), set()
    t_start, t_stop = time.time(), None

    def stop_others(why):   # exactly the processes started above: SIGTERM now, SIGKILL to whoever is still there ten seconds later
        nonlocal t_stop
        print(f"{os.path.basename(script)}: {why}; stopping the other ranks", file=sys.stderr)
        for q in alive:
            procs[q].terminate()
            stopped.add(q)
        t_stop = t_stop or time.time()

    while alive:
        for r in sorted(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.discard(r)
            if code != 0 and r not in stopped:
                worst = max(worst, code if code > 0 else 128 - code)
                stop_others(f"rank {r} exited with code {code}")
        if alive and t_stop is None and time.time() - t_start > timeout_s:
            worst = max(worst, 124)
            stop_others(f"still running after {timeout_s:.0f} s")
        if alive and t_stop is not None and time.time() - t_stop > 10.0:
            for q in alive:
                procs[q].kill()
        time.sleep(0.2)
    for t in threads:
        t.join(timeout=5)
    if len(line0) == 1:
        print(line0[0], flush=True)   # (also after a failure: a parity mismatch still reports its numbers)
    elif worst == 0:
        print(f"{os.path.basename(script)}: rank 0 printed {len(line0)} result lines", file=sys.stderr)
        worst = 1
    return worst
