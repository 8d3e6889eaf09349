"""Host side of the batched previews (no GPU): the packed primitive table, the rate-limit state ``attach_previews`` leaves
behind, and the ``TickResult`` constructor the existing callers use."""
import numpy as np

from realtime_video_analytics_32streams_amd import preview as P


def _tracks(n, w, h, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x0, y0 = float(rng.integers(0, w - 40)), float(rng.integers(0, h - 30))
        out.append({"track_id": 7 * k + 3, "class_id": int(rng.integers(0, 80)), "confidence": 0.5,
                    "bbox_xyxy": [x0 + 0.3, y0 + 0.6, min(w - 1.0, x0 + 35.5), min(h - 1.0, y0 + 25.2)]})
    return out


def test_packed_primitive_table_holds_each_frames_primitives_at_its_offsets():
    sizes = [(192, 108), (640, 360), (64, 36), (1920, 1080)]
    counts = [3, 0, 1, 11]
    prims = [P.raster_primitives(P.plan_render(wh, _tracks(n, *wh, seed=n), 75), wh) for wh, n in zip(sizes, counts)]
    rects, colors, glyphs, offs = P.pack_primitives(prims)
    assert rects.dtype == np.int32 and colors.dtype == np.uint8 and glyphs.dtype == np.int32
    assert rects.shape == (sum(len(p[0]) for p in prims), 4) and colors.shape == (len(rects), 4)
    assert glyphs.shape == (sum(len(p[2]) for p in prims), 3)
    assert len(offs) == len(prims)
    r_end = g_end = 0
    for (r, c, g), (r0, nr, g0, ng) in zip(prims, offs):
        assert (r0, g0) == (r_end, g_end), "the ranges follow each other without gaps"
        assert nr == len(r) and ng == len(g)
        assert np.array_equal(rects[r0:r0 + nr], r) and np.array_equal(colors[r0:r0 + nr], c) and np.array_equal(glyphs[g0:g0 + ng], g)
        r_end, g_end = r0 + nr, g0 + ng
    assert offs[1][1] == 0 and offs[1][3] == 0                    # the frame without tracks owns an empty range
    # a batch with no primitive at all still has well-formed (empty) arrays
    r, c, g, o = P.pack_primitives([prims[1], prims[1]])
    assert r.shape == (0, 4) and c.shape == (0, 4) and g.shape == (0, 3) and o == [(0, 0, 0, 0), (0, 0, 0, 0)]


def test_attach_previews_leaves_the_rate_limit_state_of_the_per_payload_loop(monkeypatch):
    """Scripted clock: the policy is asked once per payload that has a surface, in order, exactly like a loop of
    ``attach_preview`` -- same ``_last``, same payloads with a preview -- across a due tick, a tick inside the interval and a
    tick where only some streams are due (the rendering itself is stubbed: there is no GPU here)."""
    monkeypatch.setattr(P, "render_frame", lambda surface, tracks, q=None, policy=None, ctx=None: f"url:{surface}:{len(tracks)}:{q}")
    monkeypatch.setattr(P, "render_frames", lambda surfaces, tracks, qs, policy=None, ctx=None, batcher=None:
                        [f"url:{s}:{len(t)}:{q}" for s, t, q in zip(surfaces, tracks, qs)])
    names = ["cam0", "cam1", "cam2", "cam3"]
    script = [1000.0, 1000.04, 1000.13, 1000.26, 1000.31]

    def run(batched):
        now = [0.0]
        reads = []

        def clock():
            reads.append(now[0])
            now[0] += 0.001                                       # every read of the clock moves it: the ORDER of the questions matters
            return now[0]
        pol = P.PreviewPolicy(frame_quality=75, clock=clock)
        seen = []
        for t, base in enumerate(script):
            now[0] = base
            payloads = [{"stream": n, "frame_id": t, "tracks": _tracks((t + i) % 5, 640, 360), "is_temporal": False} for i, n in enumerate(names)]
            surfaces = [f"s{t}{i}" if not (t == 2 and i == 1) else None for i in range(len(names))]      # one frame without a surface
            if t == 3:
                pol._last["cam2"] = now[0] + 1.0                  # cam2 sent a frame through another path: not due
            if batched:
                out = P.attach_previews(payloads, surfaces, pol)
            else:
                out = [P.attach_preview(p, s, pol) for p, s in zip(payloads, surfaces)]
            seen.append([(p["stream"], p.get("frame_jpeg")) for p in out])
        return dict(pol._last), seen, len(reads)
    loop_last, loop_seen, loop_reads = run(False)
    batch_last, batch_seen, batch_reads = run(True)
    assert batch_last == loop_last and batch_reads == loop_reads
    assert batch_seen == loop_seen
    assert all(u is not None for _, u in loop_seen[0]) and all(u is None for _, u in loop_seen[1])
    assert loop_seen[2][1][1] is None and [u is None for _, u in loop_seen[3]] == [False, False, True, False]


def test_tick_result_keeps_its_four_positional_fields():
    from realtime_video_analytics_32streams_amd.pipeline import TickResult
    a = TickResult(3, {"cam0": []}, {"cam0": 0}, 0.25)
    assert (a.tick, a.tracks, a.detections_emitted, a.latency_s) == (3, {"cam0": []}, {"cam0": 0}, 0.25)
    assert a.frame_jpeg == {} and a == TickResult(3, {"cam0": []}, {"cam0": 0}, 0.25)
    b = TickResult(3, {"cam0": []}, {"cam0": 0}, 0.25)
    b.frame_jpeg["cam0"] = "data:image/jpeg;base64,"
    assert a.frame_jpeg == {}, "every result owns its own dict"
