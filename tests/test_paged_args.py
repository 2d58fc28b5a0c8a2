"""Argument and error contract of kvcompress.PagedKV / compress_paged that needs no device (the
errors that need device tensors are in tests/test_paged_gpu.py).  A pool is never copied, so every
layout the engine cannot read as it is raises ValueError; the device check comes last."""
import pytest
import torch

from kvcompress import PagedKV, compress_paged, list_methods

N_PAGES, H, P, D = 9, 3, 16, 64


def _pools(dtype=torch.bfloat16):
    return (torch.zeros(N_PAGES, H, P, D, dtype=dtype),
            torch.zeros(N_PAGES, P, H, D, dtype=dtype).permute(0, 2, 1, 3))


def _table(B=2, cols=4):
    return torch.zeros(B, cols, dtype=torch.int32)


def test_exports():
    import kvcompress
    assert "PagedKV" in kvcompress.__all__ and "compress_paged" in kvcompress.__all__
    assert "paged" not in kvcompress.__all__
    assert "h2o_attention" in list_methods()


def test_pool_layouts_that_would_need_a_copy_are_refused():
    k, v = _pools()
    with pytest.raises(ValueError, match=r"must both be \[num_pages, H, page_size, D\]"):
        PagedKV(k, v[:, :, :8], _table(), 60)
    with pytest.raises(ValueError, match=r"must both be \[num_pages, H, page_size, D\]"):
        PagedKV(k[0], v[0], _table(), 60)
    with pytest.raises(ValueError, match="of one dtype"):
        PagedKV(k, v.float(), _table(), 60)
    with pytest.raises(ValueError, match="bfloat16 / float16 / float32"):
        PagedKV(k.to(torch.float64), v.to(torch.float64), _table(), 60)
    with pytest.raises(ValueError, match="power of two"):
        PagedKV(k[:, :, :12], v[:, :, :12], _table(), 40)
    with pytest.raises(ValueError, match="k_pool needs a contiguous last dim"):
        PagedKV(torch.zeros(N_PAGES, H, P, 2 * D, dtype=torch.bfloat16)[..., ::2], v, _table(), 60)
    with pytest.raises(ValueError, match="k_pool needs a contiguous last dim"):  # 8-byte rows
        PagedKV(torch.zeros(N_PAGES, H, P, 4, dtype=torch.bfloat16),
                torch.zeros(N_PAGES, H, P, 4, dtype=torch.bfloat16), _table(), 60)
    odd = torch.zeros(N_PAGES, H, P, D + 4, dtype=torch.bfloat16)[..., :D]  # 136-byte row stride
    with pytest.raises(ValueError, match="k_pool needs .* multiples of 16 bytes"):
        PagedKV(odd, v, _table(), 60)
    with pytest.raises(ValueError, match="v_pool has stride 0"):
        PagedKV(k, k[:1].expand(N_PAGES, H, P, D), _table(), 60)


def test_block_table_and_length_rules():
    k, v = _pools()
    with pytest.raises(ValueError, match="block_table must be an int32"):
        PagedKV(k, v, _table().long(), 60)
    with pytest.raises(ValueError, match="block_table must be an int32"):
        PagedKV(k, v, _table()[0], 60)
    with pytest.raises(ValueError, match="contiguous last dim"):
        PagedKV(k, v, torch.zeros(2, 8, dtype=torch.int32)[:, ::2], 60)
    with pytest.raises(ValueError, match="holds fewer than the 5 pages of 65 rows of 16"):
        PagedKV(k, v, _table(), 65)
    with pytest.raises(ValueError, match="seq_len must be a non-negative int"):
        PagedKV(k, v, _table(), -1)
    with pytest.raises(ValueError, match="seq_len must be a non-negative int"):
        PagedKV(k, v, _table(), 60.0)
    with pytest.raises(TypeError, match="block_table must be a tensor"):
        PagedKV(k, v, [[0, 1, 2, 3]], 60)
    # everything else in order: the device check comes last (no CPU fallback)
    with pytest.raises(ValueError, match="must be on one ROCm device"):
        PagedKV(k, v, _table(), 64)


def test_compress_paged_argument_errors():
    with pytest.raises(ValueError, match="Unknown method: nope"):
        compress_paged("nope", [])
    with pytest.raises(TypeError, match="method must be a name or a compress function"):
        compress_paged(3, [])
    with pytest.raises(TypeError, match="layers must be a list of PagedKV"):
        compress_paged("fix_size_l2", [(torch.zeros(1, 1, 4, 8), torch.zeros(1, 1, 4, 8))])
    with pytest.raises(TypeError, match="layers must be a list of PagedKV"):
        compress_paged("fix_size_l2", None)
    with pytest.raises(TypeError, match="H2OAttentionManager"):
        compress_paged("h2o_attention", [], h2o_manager=object())
    with pytest.raises(ValueError, match="out='dense'"):
        compress_paged("fix_size_l2", [], out="dense")
    with pytest.raises(ValueError, match="out has 1 entries for 0 layers"):
        compress_paged("fix_size_l2", [], out=[None])
    with pytest.raises(TypeError, match="out must be"):
        compress_paged("fix_size_l2", [], out=5)
    # nothing to do: no layers, by name, by function, and "evict_for_space"
    from kvcompress.methods import fix_size_l2_compress
    assert compress_paged("fix_size_l2", []) == []
    assert compress_paged(fix_size_l2_compress, [], fix_kv_size=8) == []
    assert compress_paged("evict_for_space", [], num_coming=1, out=[]) == []
