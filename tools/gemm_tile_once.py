"""A few launches of one residual GEMM on one tile form: the workload of a per-launch counter pass (rocprofv3 --pmc FETCH_SIZE,
then WRITE_SIZE, folded by tools/pmc_traffic.py) when two tiles of the same kernel are to be compared on the same shape.
    python tools/gemm_tile_once.py M,N,K variant [raster_gm] [launches]
In place (out == resid), as the engine calls it; VISRAG_HIP_LIB picks a tagged build."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests.gpu_util import P  # noqa: E402
from visrag_amd import _lib  # noqa: E402

M, N, K = (int(x) for x in sys.argv[1].split(","))
variant = int(sys.argv[2])
gm = int(sys.argv[3]) if len(sys.argv) > 3 else 0
launches = int(sys.argv[4]) if len(sys.argv) > 4 else 4
lib = _lib.load()
Mp = (M + 255) // 256 * 256
A = torch.randn((Mp, K), device="cuda").to(torch.bfloat16)
W = (torch.randn((N, K), device="cuda") * 0.05).to(torch.bfloat16)
bias = torch.randn(N, device="cuda")
x = torch.randn((Mp, N), device="cuda")
ex = _lib.VRGemmExtras(raster_gm=gm)
s = torch.cuda.current_stream().cuda_stream
for _ in range(launches):
    _lib.check(lib.vr_op_gemm_ex(0, P(A), K, P(W), K, M, N, K, 3, P(bias), P(x), 0.25, P(x), N, None, None, 0, variant, C.byref(ex), s))
torch.cuda.synchronize()
print("done", M, N, K, "variant", variant, "raster_gm", gm, "route", lib.vr_op_gemm_route(M, N, K, 3, variant, K, K, N, C.byref(ex), 0))
