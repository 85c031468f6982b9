"""Host only: what every *_workspace_bytes function returns, against literal values recorded from the library as it was
before the layouts moved onto the one carver (csrc/workspace.h) -- never computed by the code under test.  Every layout is
written once (a struct whose constructor carves the segments), so these numbers also pin the offsets the kernels see.
The rows take every branch of every layout: the three kinds of the flex_conv forward, each refusal, the 32-bit extent
guards on either side, the hub-chunk bound of the inverted lists, a block multiple for the NMS, NetVLAD's chunk count
at both ends, and prepare's table sizes at a power of two and its limits."""
import pytest

SIZES = {
    # (B, N, K, Dp, Din, Dout)
    "dh3d_flex_conv_fwd_workspace_bytes": [
        ((1, 64, 8, 3, 32, 64), 76544),              # the bf16x6 kind
        ((2, 70, 9, 3, 64, 128), 311040),            # the fused f32 kind
        ((2, 70, 8, 3, 64, 64), 176384),
        ((2, 70, 8, 3, 128, 256), 1007872),
        ((2, 70, 3, 3, 8, 12), 34560),               # kind 2: + S, a 4-plane weight
        ((2, 70, 3, 2, 8, 12), 0),
        ((2, 70, 3, 3, 5, 12), 0),
        ((2, 70, 3, 3, 8, 10), 0),
        ((2, 1, 3, 3, 8, 12), 0),
        ((0, 70, 3, 3, 8, 12), 0),
        ((2, 70, 0, 3, 8, 12), 0),
        ((16384, 1024, 8, 3, 32, 64), 7180697600),   # bf16x6: 4 * R * Din < 2^32 ...
        ((32768, 1024, 8, 3, 32, 64), 0),            # ... and not
        ((32768, 1024, 3, 3, 8, 12), 7784629760),    # kind 2: 4 * R * Din < 2^31 ...
        ((65536, 1024, 3, 3, 8, 12), 0),             # ... and not
    ],
    "dh3d_flex_conv_bwd_workspace_bytes": [
        ((2, 70, 3, 3, 8, 12), 57088),
        ((1, 64, 8, 3, 32, 64), 133888),
        ((2, 70, 3, 3, 6, 12), 0),
        ((2, 70, 3, 3, 8, 10), 0),
        ((2, 70, 3, 2, 8, 12), 0),
        ((2, 0, 3, 3, 8, 12), 0),
    ],
    # (B, N, Din, Dout)
    "dh3d_flex_conv_pm_bwd_workspace_bytes": [
        ((2, 70, 8, 12), 37376),
        ((1, 64, 32, 64), 98304),
        ((2, 70, 6, 12), 0),
        ((2, 70, 8, 10), 0),
        ((0, 70, 8, 12), 0),
    ],
    # (B, N, K, D)
    "dh3d_flex_pool_fwd_workspace_bytes": [
        ((2, 70, 3, 8), 15616),
        ((1, 64, 8, 64), 51200),
        ((2, 70, 3, 6), 0),
        ((2, 70, 0, 8), 0),
    ],
    "dh3d_flex_deconv_fwd_workspace_bytes": [
        ((2, 70, 3, 3, 8, 12), 43264),
        ((1, 64, 8, 3, 32, 64), 107520),
        ((1, 70, 63, 3, 8, 12), 90112),              # E / kChunk steps between these two: P = 2 * (E / 64) + 1
        ((1, 70, 64, 3, 8, 12), 91392),
        ((16384, 1024, 3, 3, 8, 12), 4831840512),
        ((65536, 1024, 3, 3, 8, 12), 0),             # 4 * R * max(Din, Dout) >= 2^31
        ((2, 70, 3, 3, 6, 12), 0),
        ((2, 70, 3, 3, 8, 10), 0),
        ((2, 70, 3, 2, 8, 12), 0),
    ],
    "dh3d_flex_deconv_bwd_workspace_bytes": [
        ((2, 70, 3, 3, 8, 12), 82432),
        ((1, 64, 8, 3, 32, 64), 237568),
        ((16384, 1024, 3, 3, 8, 12), 9294581504),
        ((65536, 1024, 3, 3, 8, 12), 0),
        ((2, 70, 3, 3, 6, 12), 0),
        ((2, 70, 3, 3, 8, 10), 0),
        ((2, 70, 3, 2, 8, 12), 0),
    ],
    # (B, N, M)
    "dh3d_keypoint_nms_workspace_bytes": [
        ((2, 300, 16), 7680),
        ((2, 512, 16), 12544),                       # N a multiple of the block
        ((1, 1, 1), 768),
        ((2, 300, 4096), 7680),
        ((2, 300, 4097), 0),
        ((2, 300, 0), 0),
        ((0, 300, 16), 0),
    ],
    # (B, N, D, Cl)
    "dh3d_netvlad_workspace_bytes": [
        ((2, 100, 256, 64), 263232),                 # 2 chunks (the tile count)
        ((32, 4096, 256, 64), 16843776),             # 8 chunks (256 / B)
        ((2, 100, 128, 64), 0),
        ((2, 100, 256, 32), 0),
        ((0, 100, 256, 64), 0),
    ],
    # (B, Kd, O)
    "dh3d_netvlad_head_workspace_bytes": [
        ((2, 16384, 256), 262144),
        ((32, 16384, 256), 4194304),
        ((2, 100, 256), 4096),                       # one partly filled k slice
        ((2, 16384, 128), 0),
        ((2, 0, 256), 0),
    ],
    # (B, D, Cl, O)
    "dh3d_netvlad_tail_workspace_bytes": [
        ((2, 256, 64, 256), 393280),
        ((32, 256, 64, 256), 6292480),
        ((2, 128, 64, 256), 0),
        ((2, 256, 32, 256), 0),
        ((2, 256, 64, 128), 0),
    ],
    # (B, N, D, Cl, O)
    "dh3d_netvlad_fused_workspace_bytes": [
        ((2, 100, 256, 64, 256), 656640),
        ((32, 4096, 256, 64, 256), 23135232),
        ((2, 100, 128, 64, 256), 0),
        ((2, 100, 256, 64, 128), 0),
        ((2, 0, 256, 64, 256), 0),
    ],
    # (B, Nraw, targetnum)
    "dh3d_prepare_clouds_workspace": [
        ((2, 500, 256), 89936),
        ((1, 1, 1), 1536),
        ((2, 4096, 8192), 727520),
        ((2, 131072, 256), 23275680),
        ((2, 131073, 256), 0),
        ((2, 500, (1 << 20) + 1), 0),
        ((65536, 500, 256), 0),
        ((2, 0, 256), 0),
    ],
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_workspace_bytes(name):
    from dh3d_amd import _lib
    fn = getattr(_lib.lib(), name)
    got = [(shape, fn(*shape)) for shape, _ in SIZES[name]]
    assert got == SIZES[name]


def test_every_workspace_query_is_covered():
    """A new op with a workspace gets its rows here ("Workspaces")."""
    from dh3d_amd import _lib
    queries = {n for n in _lib.EXPORTED_SYMBOLS if n.endswith("_workspace_bytes") or n.endswith("_workspace")}
    assert queries == set(SIZES)
