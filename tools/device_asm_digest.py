"""sha256 of the gfx950 assembly of every translation unit of a checkout: `build.FLAGS` plus `-S --cuda-device-only`,
as tests/test_loader_isa_cpu.py compiles one unit.  A refactor that must leave the device code alone runs this on the
parent's checkout and on its own and compares the two files (needs hipcc, no GPU):

    python tools/device_asm_digest.py <checkout> <out.json> [<dir that keeps the .s files>]
"""
import concurrent.futures
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile


def main():
    root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    keep = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="pvae_asm_")
    os.makedirs(keep, exist_ok=True)
    spec = importlib.util.spec_from_file_location("pvae_build_of", os.path.join(root, "physicsvae_amd", "build.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    cc = B._hipcc()

    def one(u):
        s = os.path.join(keep, u.replace(".hip", ".s"))
        # (-cuid: the compilation-unit id that names one symbol is otherwise a hash of the ABSOLUTE source path, which
        #  differs between two checkouts of identical code)
        res = subprocess.run([cc] + B.FLAGS + ["-S", "--cuda-device-only", "-cuid=" + u.replace(".hip", ""),
                              os.path.join(B.CSRC, u), "-o", s],
                             capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (u, res.stderr))
        with open(s, "rb") as f:
            return u, hashlib.sha256(f.read()).hexdigest()

    with concurrent.futures.ThreadPoolExecutor(min(len(B.UNITS), os.cpu_count() or 1)) as pool:
        digests = dict(pool.map(one, B.UNITS))
    with open(out, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(digests, sort_keys=True))


if __name__ == "__main__":
    main()
