"""Machine-code bytes per conv / GEMM kernel, read from the gfx950 code objects of a build (no GPU needed).

    python tools/code_size.py [build dir, default stablediffusioneo_amd/csrc/_build]

Unbundles the device code object of conv_gemm.o and conv_halo.o and lists the size of every kernel symbol."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_sizes(obj):
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "fatbin"), os.path.join(td, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(td, "unused.o")], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={fb}", f"--output={co}"], check=True)
        sym = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", "--demangle", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for line in sym.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)", line)
        if m and ("conv_gemm_dma_kernel" in m.group(2) or "conv3x3_halo_kernel" in m.group(2) or "conv_gemm_kernel" in m.group(2)):
            name = re.sub(r"^void sdeo::", "", m.group(2))
            name = re.sub(r"\(.*$", "", name).replace(" ", "")
            out[name] = int(m.group(1))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bdir = args[0] if args else os.path.join(ROOT, "stablediffusioneo_amd", "csrc", "_build")
    sizes = {}
    for o in ("conv_gemm.o", "conv_halo.o"):
        sizes.update(kernel_sizes(os.path.join(bdir, o)))
    for name in sorted(sizes):
        print(f"{sizes[name]:8d}  {name}")
    print(f"{sum(sizes.values()):8d}  total over {len(sizes)} kernels")


if __name__ == "__main__":
    main()
