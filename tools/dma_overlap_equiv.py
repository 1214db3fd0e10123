"""SHA-256 of the outputs of the LDS-DMA kernels on fixed inputs, for a bit-for-bit comparison of
two builds of the library (MMU_LIB_PATH selects the build; one process per build):

  python tools/dma_overlap_equiv.py > new.txt;  MMU_LIB_PATH=ab/parent.so python tools/dma_overlap_equiv.py > parent.txt

Cases: the W1 weight gradient of the bench workload (M = 3072, N = 768, K = 131328 tokens, f32
accumulate), a mixed-layout data gradient with EPI_ADD_RES, the gathered 3x3 filter gradient of a
trunk map (stride 1 and 2), and attention forward / dQ / dK, dV at B = 4, L = 513, p = 0.1.
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multi-modal-uncertainty_amd"))
from src import kernels as K  # noqa: E402


def sha(t):
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(1234)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, generator=g) * scale).to(bf).to(dev)

    out = []
    M, HID, FFN = 256 * 513, 768, 3072
    dZ, A = rnd(M, FFN), rnd(M, HID)
    gW = torch.full((FFN, HID), 0.25, device=dev)
    K.gemm(dZ, FFN, False, A, HID, False, gW, HID, FFN, HID, M, epi=K.epilogue(K.EPI_STORE, accumulate=True))
    out.append(("wgrad W1 (F,F) f32 accumulate 3072x768x131328", gW))
    W1, dY = rnd(FFN, HID, scale=0.05), rnd(M, HID)
    dA = torch.empty(M, HID, dtype=bf, device=dev)
    K.gemm(dZ, FFN, True, W1, HID, False, dA, HID, M, HID, FFN, epi=K.epilogue(K.EPI_ADD_RES, residual=dY))
    out.append(("dA (T,F) add_res 131328x768x3072", dA))
    del dZ, A, dA, dY
    cl = torch.channels_last
    for s in (1, 2):
        x = rnd(32, 256, 14, 14).contiguous(memory_format=cl)
        ho = (14 - 1) // s + 1
        dy = rnd(32, 256, ho, ho).contiguous(memory_format=cl)
        dw = torch.full((256, 256, 3, 3), 0.5, device=dev).contiguous(memory_format=cl)
        K.conv_wgrad(dy, x, dw, 3, s, accumulate=True)
        out.append((f"conv 3x3 filter gradient 32x256x14x14 stride {s}", dw))
    B, L, H, p, seed = 4, 513, 12, 0.1, 7
    qkv, dO = rnd(B * L, 3 * 768), rnd(B * L, 768)
    km = torch.zeros(B, L, device=dev)
    km[: B // 2, L - L // 4:] = -10000.0
    O = torch.empty(B * L, 768, dtype=bf, device=dev)
    lse, delta = torch.empty(B * H, L, device=dev), torch.empty(B * H, L, device=dev)
    dqkv = torch.empty(B * L, 3 * 768, dtype=bf, device=dev)
    dm = K.dropmask_empty(B, L, H, dev)
    K.attention_fwd(qkv, km, O, lse, B, L, H, p, seed, dm)
    K.attention_bwd(qkv, km, O, dO, lse, delta, dqkv, B, L, H, p, seed, dm, K.attention_dbias_parts(B, L, H, dev))
    out += [("attention fwd O", O), ("attention fwd LSE", lse), ("attention fwd keep words", dm),
            ("attention dQ", dqkv[:, :768]), ("attention delta", delta), ("attention dK", dqkv[:, 768:1536]),
            ("attention dV", dqkv[:, 1536:])]
    Oi, lsei = torch.empty_like(O), torch.empty_like(lse)
    K.attention_fwd(qkv, km, Oi, lsei, B, L, H, p, seed, None)
    out.append(("attention inference-dropout fwd O", Oi.clone()))
    K.attention_fwd(qkv, km, Oi, lsei, B, L, H, 0.0, seed, None)
    out.append(("attention fwd O, p = 0", Oi.clone()))
    torch.cuda.synchronize()
    for name, t in out:
        print(f"{sha(t)}  {name}")


if __name__ == "__main__":
    main()
