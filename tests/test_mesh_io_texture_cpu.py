"""CPU: writing a textured mesh (mesh_io.write_ply with uvs= and texture_file=, mesh_io.write_texture) and reading it back through
read_ply, load_texture and load_rigid_object; and that write_ply without the new keywords writes the bytes it always wrote (a header
and a body written out by hand).  No GPU, no engine library."""
import struct

import numpy as np
import pytest

from megapose6d_amd import RigidObject, mesh_io


def _mesh():
    v = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]], np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    rng = np.random.default_rng(3)
    uvs = rng.random((4, 3, 2)).astype(np.float32)
    uvs[0, 0] = (0.0, 1.0)
    uvs[1, 1] = (np.float32(1) / np.float32(3), np.nextafter(np.float32(0.5), np.float32(1)))      # values a decimal text would not keep
    image = rng.integers(0, 256, (8, 16, 3), dtype=np.uint8)
    return v, f, uvs, image


def test_textured_ply_and_png_round_trip(tmp_path):
    v, f, uvs, image = _mesh()
    normals = mesh_io.vertex_normals(v, f).astype(np.float32)
    png = mesh_io.write_texture(tmp_path / "tet.png", image)
    ply = mesh_io.write_ply(tmp_path / "tet.ply", v, f, normals=normals, uvs=uvs, texture_file=png.name)
    assert np.array_equal(mesh_io.load_texture(png), image)
    rgba = np.concatenate([image, np.full((8, 16, 1), 255, np.uint8)], 2)
    assert np.array_equal(mesh_io.load_texture(mesh_io.write_texture(tmp_path / "rgba.png", rgba)), image)      # alpha is dropped
    head = ply.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert "comment TextureFile tet.png" in head and "property list uchar float texcoord" in head
    assert not any(line.split()[-1] in ("red", "green", "blue") for line in head if line.startswith("property"))
    raw = mesh_io.read_ply(ply)
    assert np.array_equal(raw["vertices"].astype(np.float32), v) and np.array_equal(raw["faces"], f) and raw["colors"] is None
    assert np.array_equal(raw["normals"].astype(np.float32), normals)
    assert raw["uvs"].shape == (4, 3, 2) and np.array_equal(raw["uvs"].astype(np.float32), uvs)
    assert raw["texture_path"] == tmp_path / "tet.png"
    mesh = mesh_io.load_rigid_object(RigidObject("tet", ply, mesh_units="m"))
    assert mesh["uvs"].dtype == np.float32 and np.array_equal(mesh["uvs"], uvs)
    assert (mesh["colors"] == 1).all()                                                             # white times the texture
    mips = mesh["texture_mips"]
    assert [m.shape for m in mips] == [(8, 16), (4, 8), (2, 4), (1, 2), (1, 1)] and all(m.dtype == np.uint32 for m in mips)
    assert np.array_equal(mips[0] & 0xFF, image[..., 0]) and np.array_equal((mips[0] >> 16) & 0xFF, image[..., 2])
    want = mesh_io.build_mip_chain(image)
    assert all(np.array_equal(a, b) for a, b in zip(mips, want))
    # with vertex colours as well, and a name with a blank
    ply2 = mesh_io.write_ply(tmp_path / "tet2.ply", v, f, colors=np.full((4, 3), 0.5), uvs=uvs, texture_file="my tet.png")
    mesh_io.write_texture(tmp_path / "my tet.png", image)
    raw2 = mesh_io.read_ply(ply2)
    assert raw2["texture_path"] == tmp_path / "my tet.png" and np.array_equal(raw2["uvs"].astype(np.float32), uvs)
    assert np.allclose(raw2["colors"], 128 / 255.0)


def test_the_keywords_are_refused_when_they_make_no_file(tmp_path):
    v, f, uvs, image = _mesh()
    with pytest.raises(ValueError, match="go together"):
        mesh_io.write_ply(tmp_path / "a.ply", v, f, uvs=uvs)
    with pytest.raises(ValueError, match="go together"):
        mesh_io.write_ply(tmp_path / "a.ply", v, f, texture_file="a.png")
    with pytest.raises(ValueError, match="plain file name"):
        mesh_io.write_ply(tmp_path / "a.ply", v, f, uvs=uvs, texture_file="sub/a.png")
    with pytest.raises(ValueError):
        mesh_io.write_ply(tmp_path / "a.ply", v, f, uvs=uvs[:3], texture_file="a.png")
    with pytest.raises(ValueError, match="uint8"):
        mesh_io.write_texture(tmp_path / "a.png", image.astype(np.float32))
    assert not (tmp_path / "a.ply").exists() and not (tmp_path / "a.png").exists()


def test_without_the_keywords_the_bytes_are_the_old_ones(tmp_path):
    """the file written out by hand: header line by line, then the vertex and face records"""
    v, f, _, _ = _mesh()
    normals = mesh_io.vertex_normals(v, f).astype(np.float32)
    colors = np.array([[0, 0.5, 1], [0.25, 0.25, 0.25], [1, 0, 0], [0.2, 0.4, 0.6]])
    bytes8 = np.clip(np.rint(colors * 255.0), 0, 255).astype(np.uint8)
    for with_normals, with_colors in ((True, True), (False, True), (True, False), (False, False)):
        header = ["ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y", "property float z"]
        if with_normals:
            header += ["property float nx", "property float ny", "property float nz"]
        if with_colors:
            header += ["property uchar red", "property uchar green", "property uchar blue"]
        header += ["element face 4", "property list uchar int vertex_indices", "end_header"]
        body = b""
        for k in range(4):
            body += struct.pack("<3f", *v[k])
            if with_normals:
                body += struct.pack("<3f", *normals[k])
            if with_colors:
                body += struct.pack("<3B", *bytes8[k])
        for t in f:
            body += struct.pack("<B3i", 3, *t)
        want = ("\n".join(header) + "\n").encode("ascii") + body
        path = mesh_io.write_ply(tmp_path / "plain.ply", v, f, colors=colors if with_colors else None, normals=normals if with_normals else None)
        assert path.read_bytes() == want, (with_normals, with_colors)
