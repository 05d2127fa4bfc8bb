"""vitcap_engine_score_req called on the host with made-up pointers: the two closures the *_entry_points_refuse_without_a_device
tests share.  Every refusal of the entry point comes before anything is enqueued, so none of the pointers is followed."""
import ctypes as C

BIG = 1 << 40
# the tests' short keyword names -> vitcap_score_req fields; each test adds those of its kind
COMMON = {'K': 'caps_per_image', 'ids': 'caption_ids', 'sws': 'score_ws', 'sws_bytes': 'score_ws_bytes', 'lp': 'out_logprobs',
          'out_ids': 'out_ids', 'B': 'B'}


def aligned(buf):
    """A 256-byte aligned address inside `buf` (a ctypes char array of 512 bytes or more)."""
    return C.c_void_p((C.addressof(buf) + 255) & ~255)


def entry_points(L, h, a, kind, names, **defaults):
    """-> (text, whole): fn(o, **kw) runs one request of `kind` on engine `h` with encode = 0 / 1 and returns the code.  `a` stands
    for every pointer that is not the subject of a call; `names` maps the caller's keywords of this kind to request fields,
    `defaults` are their values when a call does not give them; o is a GenOpts or None (the defaults)."""
    names = dict(COMMON, **names)

    def call(encode, o, **kw):
        f = dict(B=1, workspace=a, workspace_bytes=512, caps_per_image=1, caption_ids=a, score_ws=a, score_ws_bytes=BIG,
                 out_logprobs=a, out_ids=a)
        f.update({names[k]: v for k, v in dict(defaults, **kw).items()})
        r = L.score_req(kind=kind, encode=encode, image=a if encode else None, opts=o)
        for k, v in f.items():
            setattr(r, k, v.value if isinstance(v, C.c_void_p) else v)
        return L.lib.vitcap_engine_score_req(h, C.byref(r), None)

    return (lambda o, **kw: call(0, o, **kw)), (lambda o, **kw: call(1, o, **kw))
