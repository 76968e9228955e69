"""Condition tracks: one style / emotion vector per latent frame (DenoiserPlan.prepare(style_track=, emotion_track=) and the
window / slot forms; include/fdm_hip.h, "Condition tracks").  Host-side helpers that build a track [L, n] from keyframes; nothing here
touches the device.

A track is piecewise constant by default: the vector of a keyframe holds from its frame until the next keyframe (the first one also
covers the frames before it).  ramp = r > 0 replaces the jump at every later keyframe by a linear cross-fade over r frames centred on
it; a cross-fade row is a convex mix of the two neighbouring vectors, so the rows of a one-hot track still sum to 1.  Where a single
index is needed from such a row (the codebook of an emotion), the rule is its argmax, the first maximum (book_of)."""
import torch

from . import presets


def keyframes(L, keys, ramp=0):
    """[(frame, vector), ...] -> float32 track [L, n].  Frames ascend strictly and lie in [0, L); the first keyframe's vector also
    fills the frames before it.  ramp: frames of linear cross-fade centred on every keyframe but the first (0 = a jump)."""
    L, ramp = int(L), int(ramp)
    if L < 1:
        raise ValueError(f"L={L}")
    if ramp < 0:
        raise ValueError(f"ramp={ramp}")
    keys = [(int(f), torch.as_tensor(v, dtype=torch.float32).reshape(-1)) for f, v in keys]
    if not keys:
        raise ValueError("no keyframes")
    n = keys[0][1].numel()
    prev = -1
    for f, v in keys:
        if v.numel() != n:
            raise ValueError(f"keyframe vectors differ in width ({v.numel()} != {n})")
        if f <= prev or f >= L:
            raise ValueError(f"keyframe at frame {f}: frames must ascend strictly inside [0, {L})")
        prev = f
    out = keys[0][1].expand(L, n).clone()
    for (f, v) in keys[1:]:
        out[f:] = v
    if ramp:
        # frame i of the fade around keyframe f mixes the vectors on both sides: weight of the new vector rises linearly from
        # 1 / (ramp + 1) at f - ramp // 2 to ramp / (ramp + 1) at the fade's last frame, so no row repeats a neighbour outside the fade
        for k in range(1, len(keys)):
            f, a, b = keys[k][0], keys[k - 1][1], keys[k][1]
            lo = f - ramp // 2
            for j in range(ramp):
                i = lo + j
                if 0 <= i < L and i > keys[k - 1][0] and (k + 1 == len(keys) or i < keys[k + 1][0]):
                    w = (j + 1) / (ramp + 1)
                    out[i] = (1.0 - w) * a + w * b
    return out


def frame_rate(preset):
    """Latent frames per second of a preset: the audio encoder's 50 feature frames per second folded `pair` to one latent frame."""
    return 50.0 / presets.get(preset).pair


def from_seconds(preset, L, keys, ramp=0.0):
    """keyframes() with times: [(seconds, vector), ...] and ramp in seconds, at the preset's latent frame rate (frame = round(t * rate))."""
    r = frame_rate(preset)
    return keyframes(L, [(int(round(float(t) * r)), v) for t, v in keys], ramp=int(round(float(ramp) * r)))


def book_of(track):
    """Codebook index per row of an emotion track: argmax, the first maximum (torch.argmax; a cross-fade row between two one-hots
    takes the heavier side, the earlier index on a tie)."""
    return torch.argmax(torch.as_tensor(track, dtype=torch.float32), dim=-1)


def parse(spec, names, seconds=True):
    """"0:neutral,21.0:happy,40.0:neutral" -> [(time, one-hot), ...] for a list of condition names (or integer indices)."""
    n = len(names)
    keys = []
    for item in str(spec).split(","):
        t, _, name = item.strip().partition(":")
        name = name.strip()
        i = names.index(name) if name in names else int(name)
        if not 0 <= i < n:
            raise ValueError(f"condition {name!r} outside the {n} known")
        keys.append((float(t) if seconds else int(t), torch.eye(n)[i]))
    return keys


def from_spec(preset, L, spec, names, ramp=0.0):
    """The command-line form as a track [L, len(names)]: "0:happy,21.0:sad,40.0:happy" (seconds : name or index) at the preset's latent
    frame rate, ramp in seconds.  Keyframes at or beyond frame L lie past the end of the audio and are dropped."""
    r = frame_rate(preset)
    keys = [(t, v) for t, v in parse(spec, names) if int(round(t * r)) < int(L)]
    return from_seconds(preset, L, keys, ramp=ramp)
