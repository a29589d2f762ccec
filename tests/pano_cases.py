"""The case table of the panorama tests: ``(Hp, Wp, h, w, stride, circular)`` in latent units -> (views, min coverage, max coverage).
The counts were worked out from the rule of diffusers' ``get_views`` (tests/pano_ref.py restates it) and are pinned here, so that the
geometry code and the model cannot drift together."""

CASES = {
    (8, 8, 8, 8, 4, 0): (1, 1, 1),             # one view: the plain step
    (8, 16, 8, 8, 4, 0): (3, 1, 2),
    (12, 16, 8, 8, 4, 0): (6, 1, 4),           # two rows of views: corners 1, edges 2, the middle 4
    (8, 24, 8, 8, 8, 0): (3, 1, 1),            # stride == window: the views tile, nothing overlaps
    (8, 12, 8, 8, 4, 1): (3, 2, 2),            # circular, Wp no multiple of the window
    (8, 16, 8, 8, 4, 1): (4, 2, 2),
    (12, 16, 8, 8, 4, 1): (8, 2, 4),
    (16, 32, 16, 16, 8, 0): (3, 1, 2),         # the network tests' window
    (16, 32, 16, 16, 8, 1): (4, 2, 2),
}


def case_id(case) -> str:
    Hp, Wp, h, w, s, circ = case
    return f"{Hp}x{Wp}_win{h}x{w}_s{s}_{'circ' if circ else 'plain'}"


def divisors(n: int):
    return [d for d in range(1, n + 1) if n % d == 0]
