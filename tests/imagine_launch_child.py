"""Child process of tests/test_gpu_imagine.py::test_launch_count_is_what_the_library_states: counts the device kernels of
`HipEngine.imagine` calls from a profiler's kernel records (what a kernel trace lists) and prints them as one JSON line.  A
process of its own, so that the tracer it switches on never sits in the process that runs the rest of the suite."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import torch  # noqa: E402

import imagine_cases as IC  # noqa: E402
import infer_cases as I  # noqa: E402

DEV, SEED, OFFSET = "cuda", 11, 5


def kernels(fn):
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    out = {}
    for name in sys.argv[1:]:
        c = IC.case(name)
        eng = I.module_for(c, DEV).engine
        for mode in IC.MODES:
            for horizon, rows in ((1, 5), (3, 33)):
                d = {k: v.to(DEV) for k, v in IC.drives(c, mode, rows, horizon, supplied_z=False).items() if k != "n"}
                s0 = c.s0[:rows].to(DEV)
                run = lambda: eng.imagine(mode, s0, horizon, seed=SEED, offset=OFFSET, **d)      # noqa: E731
                run()
                out["%s/%s/%d/%d" % (name, mode, horizon, rows)] = kernels(run)
    print("IMAGINE_LAUNCHES " + json.dumps(out))


if __name__ == "__main__":
    main()
