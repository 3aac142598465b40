"""Diagnostic build (make item-counts): top-level items a wave's query evaluates, per kind of query.  GPU box:
FT_HIP_LIB=build/libfunctracer_hip_counts.so python tools/item_counts.py"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import functracer_amd as ft
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = ft.hip_lib()
ctx = ft.Context(0)
buf = (C.c_ulonglong * 48)()
for kv in filter(None, os.environ.get("FT_OPTS", "").split(",")):
    k_, v_ = kv.split("="); ctx.set_option(k_, int(v_))
for name, spp in (("bunny", 16), ("bunny-bsp12", 16), ("hollow-sphere", 16), ("hollow-sphere", 1), ("night-house-det", 16), ("sample-det", 16)):
    p = ft.parse_scene_file(os.path.join(R, "scenes", name + ".scene")); p.lower(ctx)
    jit = ft.jitter_pattern(spp)
    ctx.render(p.camera, 1920, 1080, spp, jit, fetch=False)
    lib.ft_debug_item_counts(buf, 1)
    _, st = ctx.render(p.camera, 1920, 1080, spp, jit, fetch=False)
    lib.ft_debug_item_counts(buf, 1)
    v = list(buf)
    print(f"{name} x{spp}: {st['kernel_ms']:.3f} ms (instrumented)")
    for k, label in enumerate(("closest coherent", "closest incoherent", "any coherent", "any incoherent")):
        q, items, lanes, offered = v[4 * k:4 * k + 4]
        if q:
            cull, loop = v[16 + 4 * k], v[16 + 4 * k + 1]
            print(f"   {label:20s} wave-queries {q:9d}  items evaluated / query {items / q:6.2f}  offered by the mask {offered / q:6.2f}  cycles / query: cull {cull / q:8.0f} item loop {loop / q:8.0f}")
    clk = v[16:]
    if clk[26]:
        nb = clk[26]
        print(f"   k_primary per batch ({nb} batches): total {clk[25] / nb:9.0f} cycles = ray generation {clk[22] / nb:8.0f} + closest trace {clk[23] / nb:8.0f} + shadow queries {clk[24] / nb:8.0f} + surface / shading / store / spawn {(clk[25] - clk[22] - clk[23] - clk[24]) / nb:8.0f}")
    if clk[10]:                                            # the last section split: the surface of the hits (slot 10; slot 27: batches on the one-leaf path)
        nb = clk[26]
        print(f"   surface / shading / store / spawn = surface {clk[10] / nb:8.0f} + shading / store / spawn {(clk[25] - clk[22] - clk[23] - clk[24] - clk[10]) / nb:8.0f};  one-leaf batches {clk[27]} of {nb}")
    if clk[6]:                                             # option uniform_surface: batches of an empty list that stored Colour.Zero without a ray (slot 6)
        print(f"   k_primary batches finished on an empty candidate list: {clk[6]} of {clk[26]}")
    if clk[7]:                                             # the candidate lists of the closest queries (k_block_lists): slots 2, 3, 7
        lq = clk[7]
        print(f"   closest queries through a block's list {lq} ({lq / max(v[0], 1):.2f} per coherent closest wave-query): entries offered / query {clk[2] / lq:6.2f}  "
              f"past the wave's tests = triangles tested {clk[3] / lq:6.2f}")
        if clk[11]:                                        # option edge_cull (slot 11; a library from before it leaves the slot at 0)
            print(f"      entries kept by the rectangles / query {clk[11] / lq:6.2f}  kept by the edges {clk[3] / lq:6.2f}")
    if clk[14] and clk[31]:                                # the shadow grids' entries: slots 14 (rectangles) and 15 (edges)
        print(f"   shadow-grid entries per walk: kept by the rectangles {clk[14] / clk[31]:6.2f}  kept by the edges {clk[15] / clk[31]:6.2f}")
    if clk[31]:
        walks, qa = clk[31], v[8]
        nb = clk[26] or 1
        print(f"   coherent any-hit mesh walks {walks} ({walks / max(qa, 1):.2f} per shadow wave-query): nodes / walk {clk[28] / walks:7.2f}  triangles / walk {clk[29] / walks:7.2f}  "
              f"leaf cycles / walk {clk[30] / walks:8.0f};  per k_primary batch: shadow {clk[24] / nb:8.0f} = leaves {clk[30] / nb:8.0f} + walk and the rest {(clk[24] - clk[30]) / nb:8.0f}")
    if clk[21]:
        nb = clk[21]
        print(f"   k_bounce per batch ({nb} batches): total {clk[20] / nb:9.0f} cycles = closest trace {clk[16] / nb:8.0f} + surface {(clk[17] - clk[16]) / nb:8.0f} + shadow queries {clk[18] / nb:8.0f} + shading / store / spawn {clk[19] / nb:8.0f}")
