"""One sha256 over the loss and every gradient of one deterministic forward + backward, for comparing two builds of the library.

    HSIMAE_LIB=/path/to/libhsimae_hip.so python scripts/step_digest.py KIND [NAME=VALUE]

KIND is base, base_fp8 or large: the shapes of tests/test_gpu_sched.py::make (dim 128 / 48 bands / N = 32, dim 256 / 96 bands /
N = 16), data seed 21, the first mask grid.  NAME=VALUE is put into the environment before the library is loaded (a schedule
switch, or HSIMAE_TWO_STREAMS=0).  `model.deterministic` makes the gradients independent of the order the workgroups commit in,
so two libraries with the same kernels and the same wiring print the same line.
"""
import contextlib
import hashlib
import io
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main(kind, switch=None):
    if switch:
        name, value = switch.split("=", 1)
        os.environ[name] = value
    import torch
    from hsimae_amd import HSIMAE

    torch.manual_seed(3)
    dim, heads, bands = (256, 16, 96) if kind == "large" else (128, 8, 48)
    with contextlib.redirect_stdout(io.StringIO()):
        m = HSIMAE(img_size=9, patch_size=3, in_chans=1, bands=bands, b_patch_size=8, embed_dim=dim, depth=12, num_heads=heads,
                   s_depth=9, decoder_embed_dim=64, decoder_depth=8, decoder_num_heads=8, norm_pix_loss=True, trunc_init=True)
    m = m.to("cuda:0")
    if kind == "base_fp8":
        m.set_precision("fp8")
    m.deterministic = True
    N = 16 if kind == "large" else 32
    g = torch.Generator().manual_seed(21)
    x = torch.rand(N, 1, bands, 9, 9, generator=g).to("cuda:0")
    T = bands // 8
    noise = (torch.rand(N, T, generator=g), torch.rand(N, 9, generator=g))
    loss = m(x, 0.75, noise=noise, grid=HSIMAE.grid_candidates(T, 9, 0.75)[0])[0]
    loss.backward()
    torch.cuda.synchronize()
    h = hashlib.sha256(struct.pack("<d", loss.item()))
    ngrad = 0
    for name, p in m.named_parameters():
        if p.grad is not None:
            h.update(name.encode())
            h.update(p.grad.detach().cpu().contiguous().numpy().tobytes())
            ngrad += 1
    print(f"{kind} {switch or '-'} loss={loss.item():.9g} grads={ngrad} sha256={h.hexdigest()}")


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or sys.argv[1] not in ("base", "base_fp8", "large"):
        sys.exit(__doc__)
    main(*sys.argv[1:])
