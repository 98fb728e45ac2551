"""GPU: ``seam_repack_many_f32`` (every fp32 weight-pack form of a table of jobs in one launch) against the per-layer ABI calls, byte
for byte.  Both routes write into buffers pre-filled with the same poison and 64 spare elements behind the pack, so an unwritten
or over-written byte shows.  The weights-stationary form has no per-layer kernel: its reference is what ``ops.pack_conv`` computes
in torch, ``weight.reshape(K, C) * scale[:, None]``.

One case of the issue's list, ``(96, 40, 3, 3, 40, 0)``, is refused by ``seam_pack_conv_weight_f32`` (a row of 40 stored channels
is neither shorter than a 32-float chunk nor a multiple of it); the table route has to refuse it the same way, and the same layer
with 64 stored channels covers "K not a multiple of 64, rows padded to 128"."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SPARE = 64

# (K, Cin, R, S, Cstore, mode) -> forms
IGEMM, WINO, WINO24, PC, SW, SPLIT3, NARROW = range(7)
JOBS = [
    ((64, 3, 7, 7, 4, 0), (IGEMM, SPLIT3)),                      # the stem
    ((64, 12, 4, 4, 12, 0), (IGEMM,)),                           # the stem on the space-to-depth frame
    ((15, 256, 1, 1, 256, 0), (IGEMM, NARROW, SW)),              # the RPN head's logits + deltas
    ((96, 40, 3, 3, 64, 0), (IGEMM, WINO, WINO24, SPLIT3)),      # K not a multiple of 64: rows padded to 128
    ((256, 64, 1, 1, 64, 0), (IGEMM, SW, SPLIT3)),
    ((128, 128, 3, 3, 128, 0), (IGEMM, WINO, WINO24, SPLIT3)),
    ((512, 256, 1, 1, 256, 0), (IGEMM, PC, SW, SPLIT3)),
    ((64, 32, 1, 1, 32, 2), (IGEMM,)),                           # input-gradient weights of a [32, 64, 1, 1] conv (Cout = 32)
    ((96, 64, 3, 3, 64, 2), (IGEMM, WINO, WINO24)),              # ... and of a [64, 96, 3, 3] conv
    ((1024, 256, 1, 1, 256, 1), (IGEMM,)),                       # ConvTranspose2d [256, 256, 2, 2]
    ((32, 8, 3, 3, 8, 0), (WINO,)),                              # 64 items: less than one block
    ((3, 5, 1, 1, 5, 0), (SW,)),                                 # 15 items
]
PAIRS = [(spec, form) for spec, forms in JOBS for form in forms]


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return C.c_void_p(t.data_ptr())


def poisoned(n, dtype=torch.float32):
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xCD, dtype=torch.uint8, device=DEV).view(dtype)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


_W = {}


def weights(spec):
    """(source weight in its PyTorch layout, per-row scale), made once per job"""
    if spec not in _W:
        K, cin, R, S, cs, mode = spec
        g = torch.Generator().manual_seed(hash(spec) % (1 << 31))
        shape = {0: (K, cin, R, S), 1: (cin, K // 4, 2, 2), 2: (cin, K, R, S)}[mode]
        _W[spec] = (torch.randn(shape, generator=g).to(DEV).contiguous(), (torch.rand(K, generator=g) + 0.5).to(DEV))
    return _W[spec]


def dst_elems(spec, form):
    K, cin, R, S, cs, mode = spec
    L = lib()
    if form == IGEMM:
        return L.seam_conv_rows_padded(K) * L.seam_conv_kred(cs, R, S), torch.float32
    if form == SPLIT3:
        return L.seam_conv_rows_padded(K) * L.seam_conv_kred(cs, R, S) * 3, torch.bfloat16
    if form == WINO:
        return int(L.seam_wino_weight_floats(K, cs)), torch.float32
    if form == WINO24:
        return int(L.seam_wino24_weight_floats(K, cs)), torch.float32
    if form == NARROW:
        return 64 * cs, torch.float32
    return K * cs, torch.float32          # PC, SW


_REF = {}


def reference(spec, form):
    """the per-layer route's bytes, computed once and never written again"""
    if (spec, form) not in _REF:
        from seam_match_rcnn_amd import _native
        K, cin, R, S, cs, mode = spec
        w, scale = weights(spec)
        n, dt = dst_elems(spec, form)
        out = poisoned(n + SPARE, dt)
        L = lib()
        if form == IGEMM:
            rc = L.seam_pack_conv_weight_f32(ptr(w), ptr(out), K, cin, R, S, cs, mode, stream())
        elif form == SPLIT3:
            tmp = torch.empty(n // 3, dtype=torch.float32, device=DEV)
            rc = L.seam_pack_conv_weight_sx(ptr(w), ptr(out), ptr(tmp), K, cin, R, S, cs, mode, stream())
        elif form == WINO:
            rc = L.seam_pack_conv_weight_wino_f32(ptr(w), ptr(out), K, cin, cs, mode, stream())
        elif form == WINO24:
            rc = L.seam_pack_conv_weight_wino24_f32(ptr(w), ptr(out), K, cin, cs, mode, stream())
        elif form == NARROW:
            rc = L.seam_pack_linear_narrow_f32(ptr(w), ptr(out), K, cs, stream())
        elif form == PC:
            rc = L.seam_pack_conv1x1_pc_f32(ptr(w), ptr(out), K, cs, stream())
        else:
            rc = 0
            out[:n] = (w.reshape(K, cin) * scale[:, None]).reshape(-1)
        _native.check(rc, f"per-layer pack of {spec} form {form}")
        torch.cuda.synchronize()
        _REF[(spec, form)] = out
    return _REF[(spec, form)]


def run_table(pairs):
    """one ``seam_repack_many_f32`` launch over ``pairs``; -> the destination buffers"""
    from seam_match_rcnn_amd import _native
    from seam_match_rcnn_amd.ops import _upload
    outs, jobs = [], []
    for spec, form in pairs:
        K, cin, R, S, cs, mode = spec
        w, scale = weights(spec)
        n, dt = dst_elems(spec, form)
        out = poisoned(n + SPARE, dt)
        outs.append(out)
        one = form in (PC, SW, NARROW)
        jobs.append(_native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), scale=scale.data_ptr() if form == SW else None, form=form,
                                      K=K, Cin=cin, R=3 if form in (WINO, WINO24) else 1 if one else R,
                                      S=3 if form in (WINO, WINO24) else 1 if one else S, Cstore=cs, mode=mode))
    arr = (_native.RepackJob * len(jobs))(*jobs)
    blocks = int(lib().seam_repack_layout(arr, len(jobs)))
    assert blocks > 0, f"seam_repack_layout refused job {-1 - blocks}"
    assert arr[0].first_block == 0 and all(arr[i].first_block + arr[i].n_blocks == arr[i + 1].first_block for i in range(len(jobs) - 1))
    assert arr[len(jobs) - 1].first_block + arr[len(jobs) - 1].n_blocks == blocks
    table = _upload(arr, DEV)
    _native.check(lib().seam_repack_many_f32(ptr(table), len(jobs), blocks, stream()), "seam_repack_many_f32")
    torch.cuda.synchronize()
    return outs, arr


@pytest.mark.parametrize("spec,form", PAIRS, ids=[f"{'x'.join(map(str, s))}-form{f}" for s, f in PAIRS])
def test_a_table_of_one_job_writes_the_per_layer_bytes(spec, form):
    (out,), arr = run_table([(spec, form)])
    assert same_bytes(out, reference(spec, form))
    assert arr[0].items > 0 and arr[0].n_blocks == min(512, (arr[0].items + 255) // 256)


def test_first_and_last_jobs_smaller_than_one_block():
    small_a, small_b = ((32, 8, 3, 3, 8, 0), WINO), ((3, 5, 1, 1, 5, 0), SW)
    pairs = [small_a, ((128, 128, 3, 3, 128, 0), WINO24), ((512, 256, 1, 1, 256, 0), PC), ((64, 3, 7, 7, 4, 0), SPLIT3), small_b]
    outs, arr = run_table(pairs)
    assert arr[0].n_blocks == 1 and arr[len(pairs) - 1].n_blocks == 1 and arr[0].items < 256 and arr[len(pairs) - 1].items < 256
    for out, (spec, form) in zip(outs, pairs):
        assert same_bytes(out, reference(spec, form)), (spec, form)


def test_sixty_jobs_of_mixed_sizes_in_one_launch():
    pairs = [PAIRS[(11 * i) % len(PAIRS)] for i in range(60)]           # 11 and len(PAIRS) are coprime: every pair, interleaved
    assert set(pairs) == set(PAIRS)
    outs, arr = run_table(pairs)
    for out, (spec, form) in zip(outs, pairs):
        assert same_bytes(out, reference(spec, form)), (spec, form)


def test_what_the_per_layer_entry_refuses_the_table_refuses():
    from seam_match_rcnn_amd import _native
    K, cin, R, S, cs, mode = spec = (96, 40, 3, 3, 40, 0)           # 40 stored channels: not a multiple of the 32-float chunk
    w = torch.zeros((K, cin, R, S), device=DEV)
    out = poisoned(128 * 9 * 64 + SPARE)
    before = out.clone()
    assert lib().seam_pack_conv_weight_f32(ptr(w), ptr(out), K, cin, R, S, cs, mode, stream()) != 0
    ok = _native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=IGEMM, K=64, Cin=3, R=7, S=7, Cstore=4, mode=0)
    bad = [_native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=IGEMM, K=K, Cin=cin, R=R, S=S, Cstore=cs, mode=mode),
           _native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=WINO, K=100, Cin=64, R=3, S=3, Cstore=64, mode=0),
           _native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=PC, K=256, Cin=192, R=1, S=1, Cstore=192, mode=0),
           _native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=NARROW, K=17, Cin=256, R=1, S=1, Cstore=256, mode=0),
           _native.RepackJob(src=None, dst=out.data_ptr(), form=SW, K=4, Cin=4, R=1, S=1, Cstore=4, mode=0),
           _native.RepackJob(src=w.data_ptr(), dst=out.data_ptr(), form=9, K=4, Cin=4, R=1, S=1, Cstore=4, mode=0)]
    for b in bad:
        arr = (_native.RepackJob * 2)(ok, b)
        assert lib().seam_repack_layout(arr, 2) == -2
    assert lib().seam_repack_many_f32(None, 0, 0, stream()) == 0 and lib().seam_repack_many_f32(None, 1, 1, stream()) != 0
    torch.cuda.synchronize()
    assert same_bytes(out, before)
