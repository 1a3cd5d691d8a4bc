"""The step-plan table: shapes and FusedStep arguments with the whole StepPlan
expected of pipeline.step_plan on a 256-CU chip.  tests/test_host_logic.py
holds step_plan to it; tests/frames16_cases.py takes its four real shapes for
the plan tests of the 16-bit fronts.  Plain helper module: no test is
collected from it.
"""


def _plan_cases():
    """(shape, arguments) -> the whole StepPlan on a 256-CU chip.  D = 300
    throughout (the fp16 split applies).  The expectations restate the
    constructor's boolean precedence as it stood before step_plan existed."""
    c3 = dict(n=1_000_000, t=40, a=300, vd=300, V=400_000)
    mosi = dict(n=1284, t=20, a=76, vd=48, V=3016)
    pom = dict(n=100, t=1089, a=300, vd=300, V=7763)
    mid = dict(n=700, t=40, a=300, vd=300, V=5000)
    one700, three700 = ((0, 700),), ((0, 256), (256, 512), (512, 700))
    return [
        # configs[3]: fused front, int8 Gram, the removal its own launch
        (c3, {}, ("fused", False, "i8", "front", False, ((0, 1_000_000),), 1_000_192, True)),
        (c3, dict(gram_kind="f64"),
         ("fused", False, "f64", "front", False, ((0, 1_000_000),), 1_000_192, True)),
        (mosi, {}, ("narrow_fused", False, "f64", "front", False, ((0, 1284),), 1536, True)),
        (mosi, dict(narrow_fused=False),
         ("stream", False, "f64", "fork", True, ((0, 1284),), 1536, True)),
        # a few long rows: split stream (n <= CUs, t > 64), forked projection
        (pom, {}, ("stream", True, "f64", "fork", True, ((0, 100),), 256, True)),
        ({**pom, "n": 256}, {}, ("stream", True, "f64", "fork", True, ((0, 256),), 256, True)),
        ({**pom, "n": 257}, {}, ("stream", False, "f64", "fork", True, ((0, 257),), 512, True)),
        (pom, dict(split_stream=False),
         ("stream", False, "f64", "fork", True, ((0, 100),), 256, True)),
        # the two-kernel step: forked up to FORK_PROJECTION_MAX_ROWS rows,
        # projection + removal in one kernel above or with the fork refused
        (mid, dict(stream_project=False), ("stream", False, "f64", "fork", True, one700, 768, True)),
        (mid, dict(stream_project=False, fork_projection=False),
         ("stream", False, "f64", "remove", True, one700, 768, True)),
        ({**mid, "n": 5000}, dict(stream_project=False),
         ("stream", False, "f64", "remove", True, ((0, 5000),), 5120, True)),
        (mid, dict(stream_project=False, split_projection=False),
         ("stream", False, "f64", "fork", False, one700, 768, True)),
        (mid, dict(fuse_remove=False), ("fused", False, "f64", "front", False, one700, 768, True)),
        (mid, dict(fuse_remove=False, stream_project=False),
         ("stream", False, "f64", "chunk", True, one700, 768, True)),
        # chunks: the plain stream kernel, Gram partials, no split-K projection
        (mid, dict(chunks=3), ("stream", False, "parts", "chunk", False, three700, 256, True)),
        (mid, dict(chunks=3, gram_kind="i8"),
         ("stream", False, "parts", "chunk", False, three700, 256, True)),
        # fewer utterances than features: one chunk, but the fused front
        # kernels stay off because more than one chunk was asked for
        ({**mid, "n": 200}, dict(chunks=4),
         ("stream", False, "f64", "fork", True, ((0, 200),), 256, True)),
        (mid, dict(npc=2), ("fused", False, "f64", "front", False, one700, 768, True)),
        (mid, dict(npc=2, stream_project=False),
         ("stream", False, "f64", "chunk", True, one700, 768, True)),
        # a forced Gram below GRAM_I8_MIN_ROWS; the default follows n_total
        (mid, dict(gram_kind="i8"), ("fused", False, "i8", "front", False, one700, 768, True)),
        ({**mid, "n": 20_000, "n_total": 40_000}, {},
         ("fused", False, "i8", "front", False, ((0, 20_000),), 20_224, True)),
    ]
