"""Run-to-run determinism of the full GAN iteration: prints the losses of a few iterations as exact hex floats.  Two runs of the
same build and flags must print identical lines; so must SRK_D_OVERLAP=0 and =1 (the schedule must not change a single bit)."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
train = importlib.import_module("super-resolution_amd.train")
torch.manual_seed(0)
st = train.Stepper(workload="gan", res_blocks=23, device=torch.device("cuda"), hr=256, factor=4)
g = torch.Generator().manual_seed(0)
pool = [(10 * torch.rand(32, 1, 256, 256, generator=g) * (torch.rand(32, 1, 256, 256, generator=g) < 0.1)).cuda() for _ in range(4)]
for it in range(int(os.environ.get("ITERS", 24))):
    hr = pool[it % len(pool)]
    lr = torch.nn.functional.avg_pool2d(hr, 4) * 16
    out = st.step(lr, hr)
    if it in (0, 1, 3, 7, 15, 23, 59, 99, 149):
        v = st.loss_scalars(out)
        print(it, float(v["g_loss"]).hex(), float(v["d_loss_def"]).hex(), float(v["d_loss_pow"]).hex(), flush=True)
