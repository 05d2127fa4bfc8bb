"""Test helper of tests/test_hip_rollout.py: the staged engine calls around vitcap_engine_encode_maps, made directly through ctypes
on the model's own engine and workspace."""
import ctypes as C

import torch


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def encode_maps(model, img, o, mask, per_head, maps, maps_bytes=None, ws=None):
    """vitcap_engine_encode_maps on slot 0's workspace (or `ws`) -> (rc, workspace, bytes)."""
    from vitcap_amd._lib import lib
    B = img.shape[0]
    if ws is None:
        ws, need = model._workspace(B, img.device, 0, o)
    else:
        need = ws.numel()
    if maps_bytes is None:
        maps_bytes = maps.numel() * 4 if maps is not None else 0
    rc = lib.vitcap_engine_encode_maps(model._engine, _p(img), int(img.dtype == torch.bfloat16), B, C.byref(o), _p(ws), need, mask, per_head,
                                       _p(maps), maps_bytes, _s())
    return rc, ws, need


def encode(model, img, o, ws, need):
    """vitcap_engine_encode -> rc."""
    from vitcap_amd._lib import lib
    return lib.vitcap_engine_encode(model._engine, _p(img), int(img.dtype == torch.bfloat16), img.shape[0], C.byref(o), _p(ws), need, _s())


def prefill_and_decode(model, B, o, ws, need):
    """vitcap_engine_prefill, then vitcap_engine_decode -> (rc of each, ids (B, 1, L), logprobs (B, 1))."""
    from vitcap_amd._lib import lib
    rc_p = lib.vitcap_engine_prefill(model._engine, B, C.byref(o), _p(ws), need, _s())
    ids = torch.empty((B, 1, o.max_length), dtype=torch.int64, device=ws.device)
    lp = torch.empty((B, 1), dtype=torch.float32, device=ws.device)
    rc_d = lib.vitcap_engine_decode(model._engine, B, C.byref(o), _p(ws), need, _p(ids), _p(lp), None, _s())
    return rc_p, rc_d, ids, lp
