"""One timed run of blvm_wavenet_decode (zero start) through the raw C ABI of the library given on the command line."""
import ctypes, hashlib, json, sys
import torch
sys.path.insert(0, "benchmarking-lvms_amd")
from blvm import _hip
from blvm.models import WaveNet
from blvm.modules.distributions import DiscretizedLogisticMixtureDense

path, tag = sys.argv[1], sys.argv[2]
lib = ctypes.CDLL(path)
ci = ctypes.c_int
for name in ("blvm_wavenet_decode_scratch_floats", "blvm_wavenet_decode"):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _hip.SIGNATURES[name]
torch.manual_seed(0)
C, B, N = 64, 16, 2000
m = WaveNet(likelihood=DiscretizedLogisticMixtureDense(C, 1, num_mix=10, num_bins=2**16), n_layers=10, n_stacks=5, res_channels=C).cuda()
rs, lik = m.res_stack, m.likelihood
hw, hb = lik.params.weight, lik.params.bias
parts = [m.causal.conv.weight, m.causal.conv.bias, rs.in_transform.weight, rs.in_transform.bias, *(p for b in rs.res_blocks for p in b.kernel_params()),
         m.out_transform.linear.weight, m.out_transform.linear.bias, hw, hw.new_zeros(2, C), hb, hb.new_zeros(2)]
packed = torch.cat([p.detach().float().reshape(-1) for p in parts])
dil = (ci * 50)(*rs.dilations)
scratch = torch.empty(lib.blvm_wavenet_decode_scratch_floats(dil, 50, B, C, C), device="cuda")
g = torch.Generator(device="cuda").manual_seed(1)
u = torch.empty(N, B, 10, device="cuda").uniform_(1e-5, 1 - 1e-5, generator=g)
v = torch.empty(N, B, device="cuda").uniform_(1e-8, 1 - 1e-8, generator=g)
x = torch.zeros(B, N, device="cuda")

def run(n):
    rc = lib.blvm_wavenet_decode(packed.data_ptr(), dil, 50, B, C, C, C, 10, n, rs.res_blocks[0].inv_std, 1.0 / m.variance_scale, -7.0,
                                 u.data_ptr(), v.data_ptr(), scratch.data_ptr(), x.data_ptr(), None)
    assert rc == 0

run(200)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(); run(N); e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1)
print(json.dumps(dict(tag=tag, entry="blvm_wavenet_decode", B=B, frames=N, ms_total=round(ms, 3), ms_per_frame=round(ms / N, 5),
                      sha=hashlib.sha1(x.cpu().numpy().tobytes()).hexdigest()[:12])), flush=True)
