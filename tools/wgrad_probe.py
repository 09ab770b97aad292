import sys, torch
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from persia_amd.ops import native
C = native()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
for (M, N, K) in [(512,256,224),(512,256,256),(1024,256,224),(512,64,64),(512,256,32),(4096,256,224),(512,1024,224)]:
    dC = (torch.randn(M, N, device=dev) * 0.1).to(torch.bfloat16).contiguous()
    A = (torch.randn(M, K, device=dev) * 0.1).to(torch.bfloat16).contiguous()
    dW = C.wgrad(dC, A)
    ref = dC.float().t() @ A.float()
    err = (dW - ref).abs().max().item()
    print(f"M{M} N{N} K{K} {C.wgrad_config(M, N, K)} err {err:.4f}", flush=True)
