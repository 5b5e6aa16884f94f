"""The wiring record of a node (engine.Wiring, made once in Graph.add) and the index the planning passes read
(graph_plan.WiringIndex): one definition of "output" -- the tensors the node's constructor made -- for every preset, on CPU
(no kernels run: MultiBoxPrior, the one operator a graph BUILD calls, is stubbed)."""
import pytest
import torch

from dspnet_amd import engine as E
from dspnet_amd import graph_plan
from dspnet_amd import operator as op
from dspnet_amd.symbol import multitask_symbol_builder as B
from dspnet_amd.symbol import multitask_symbol_factory as F


@pytest.fixture()
def stub_prior(monkeypatch):
    def fake_prior(data, sizes, ratios, **kw):
        H, W = data if isinstance(data, tuple) else data.shape[-2:]
        return torch.zeros(1, H * W * (len(sizes) + len(ratios) - 1), 4)
    monkeypatch.setattr(op, "MultiBoxPrior", fake_prior)


def held(node):
    """(attribute, engine Tensor / Param) of everything the node holds NOW, walked independently of the record"""
    for k, v in vars(node).items():
        for t in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else (v,)):
            if isinstance(t, (E.Tensor, E.Param)):
                yield k, t


@pytest.mark.parametrize("network", ["resnet-50", "vgg16_reduced", "inceptionv3", "resnet101"])
@pytest.mark.parametrize("train", [True, False])
def test_every_tensor_has_one_writer_and_every_held_tensor_one_role(stub_prior, network, train):
    f = F.get_multi_symbol_train if train else F.get_multi_symbol
    g = f(network, 512, num_classes=8, batch_size=1, device=torch.device("cpu")).g
    index = graph_plan.WiringIndex(g.nodes)
    made = {}
    for i, n in enumerate(g.nodes):
        for t in n.wiring.outputs:
            assert id(t) not in made, "%s is made by nodes %d and %d" % (t.name, made[id(t)], i)
            made[id(t)] = i
    known = {id(t) for t in g.all_tensors}
    assert set(made) <= known
    assert index.writer == made                       # exactly one writer per node-made tensor, and it is that node
    assert len(made) > len(g.nodes) // 2
    for i, n in enumerate(g.nodes):
        outs = {id(t) for t in n.wiring.outputs}
        reads = {id(t) for _, t in n.wiring.reads}
        assert not (outs & reads), "node %d lists a tensor as output and as read" % i
        # after finalize() (which re-points a convolution's x_raw): the record still is what the node holds
        now = list(held(n))
        assert {(k, id(t)) for k, t in now if isinstance(t, E.Tensor) and id(t) not in outs} == {(k, id(t)) for k, t in n.wiring.reads}
        assert {id(t) for _, t in now if isinstance(t, E.Tensor)} <= outs | reads
        assert {id(p) for _, p in now if isinstance(p, E.Param)} == {id(p) for p in n.wiring.params}
        for k, t in n.wiring.reads:
            assert (i, k) in index.readers[id(t)]
    for tid, rs in index.readers.items():
        order = [i for i, _ in rs]
        assert order == sorted(order) and index.first_reader(next(t for t in g.all_tensors if id(t) == tid)) == order[0]
        assert tid not in made or made[tid] < rs[0][0], "a tensor is read before the node that writes it"


def test_tensors_in_dict_list_and_tuple_are_recorded():
    class Holder(E.Node):
        def __init__(self, g, a, b, c):
            self.by_name, self.many, self.pair = {"a": a}, [b], (c, None)
            self.w = {"w": g.param("holder_w", (4,), E.init_zeros)}
            self.out = g.tensor((1, 4), "holder_out")

    g = E.Graph(torch.device("cpu"))
    a, b, c = (g.tensor((1, 4), s) for s in "abc")
    n = g.add(Holder(g, a, b, c))
    assert n.wiring.outputs == [n.out]
    assert n.wiring.reads == [("by_name", a), ("many", b), ("pair", c)]
    assert n.wiring.params == [g.params["holder_w"]]
    index = graph_plan.WiringIndex(g.nodes)
    assert index.writer == {id(n.out): 0} and index.reader_nodes(b) == {0} and index.reader_nodes(b, skip=("many",)) == set()
    assert index.first_reader(n.out) is None


def test_identity_avgpool_and_detection_read_what_they_do_not_make(stub_prior):
    g = E.Graph(torch.device("cpu"))
    x = g.tensor((1, 4, 4, 4), "x")
    pool = g.add(E.AvgPool(g, x, "pool1", 1))
    assert pool.out is x
    assert pool.wiring.outputs == [] and {t for _, t in pool.wiring.reads} == {x}
    assert ("x", x) in pool.wiring.reads

    net = F.get_multi_symbol("resnet-50", 512, num_classes=8, batch_size=1, device=torch.device("cpu"))
    (det,) = [n for n in net.g.nodes if isinstance(n, B.Detection)]
    assert ("cls_prob", det.cls_prob) in det.wiring.reads and det.cls_prob not in det.wiring.outputs
    index = graph_plan.WiringIndex(net.g.nodes)
    assert isinstance(net.g.nodes[index.writer[id(det.cls_prob)]], (B.ClsSoftmaxActivation, B.ClsSoftmaxOutput))
