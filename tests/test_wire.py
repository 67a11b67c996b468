"""Wire compatibility of the programmatic federated.proto with the reference.

What the reference's generated protobuf module declares and serializes is recorded in
tests/golden/wire_reference.json (tools/record_reference_golden.py): package, syntax, messages and
fields, service methods, and the bytes of sample messages.  Our descriptor and bytes must equal
them, and a peer built from that record alone (its own descriptor pool, plain grpc calls -- what
a generated stub / servicer does) must talk to our servers and stubs.
"""
import base64
import json
import re
from pathlib import Path

import grpc
import pytest
from google.protobuf import descriptor_pb2, descriptor_pool, message_factory

from fedmi.wire import proto as P

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "wire_reference.json"

SAMPLES = [("TrainRequest", dict(rank=1, world=2)), ("TrainReply", dict(message="abc")),
           ("SendModelRequest", dict(model="QUJD")), ("SendModelReply", dict(reply="success")),
           ("PingRequest", dict(req="1")), ("PingResponse", dict(value=1)),
           ("HeartBeatResponse", dict(status=1)), ("Request", {})]


class _RefPeer:
    """The reference side of the wire, from the recorded facts: message classes of its own descriptor
    pool, a stub of plain unary-unary calls and a servicer registration on the recorded method paths."""

    def __init__(self, rec: dict):
        self.rec = rec
        fdp = descriptor_pb2.FileDescriptorProto(name=rec["name"], package=rec["package"], syntax=rec["syntax"])
        for m in rec["messages"]:
            mt = fdp.message_type.add(name=m["name"])
            for fname, num, ftype, label in m["fields"]:
                mt.field.add(name=fname, number=num, type=ftype, label=label)
        pool = descriptor_pool.DescriptorPool()
        pool.Add(fdp)
        self.service = f'{rec["package"]}.{rec["service"]["name"]}'
        self.methods = {name: (self._cls(pool, i), self._cls(pool, o)) for name, i, o in rec["service"]["methods"]}
        for m in rec["messages"]:
            setattr(self, m["name"], self._cls(pool, f'.{rec["package"]}.{m["name"]}'))

    @staticmethod
    def _cls(pool, full_name: str):
        return message_factory.GetMessageClass(pool.FindMessageTypeByName(full_name.lstrip(".")))

    def stub(self, channel):
        class Stub:
            pass

        s = Stub()
        for rpc, (req, resp) in self.methods.items():
            setattr(s, rpc, channel.unary_unary(f"/{self.service}/{rpc}", request_serializer=req.SerializeToString,
                                                response_deserializer=resp.FromString))
        return s

    def add_servicer_to_server(self, servicer, server):
        handlers = {rpc: grpc.unary_unary_rpc_method_handler(getattr(servicer, rpc), request_deserializer=req.FromString,
                                                             response_serializer=resp.SerializeToString)
                    for rpc, (req, resp) in self.methods.items() if hasattr(servicer, rpc)}
        server.add_generic_rpc_handlers((grpc.method_handlers_generic_handler(self.service, handlers),))


@pytest.fixture(scope="module")
def ref():
    return _RefPeer(json.loads(GOLDEN.read_text()))


def test_messages_and_fields_match_proto_file():
    text = (ROOT / "proto" / "federated.proto").read_text()
    for name, fields in P.MESSAGES.items():
        m = re.search(r"message\s+%s\s*\{([^}]*)\}" % name, text)
        assert m, name
        body = m.group(1)
        for fname, num, _ in fields:
            assert re.search(r"\b%s\s*=\s*%d\s*;" % (fname, num), body), (name, fname)
    for rpc, (req, resp) in P.METHODS.items():
        assert re.search(r"rpc\s+%s\s*\(\s*%s\s*\)\s*returns\s*\(\s*%s\s*\)" % (rpc, req, resp), text), rpc
    assert "package federated;" in text


def test_roundtrip_and_string_payload():
    r = P.TrainRequest(rank=3, world=8)
    assert P.TrainRequest.FromString(r.SerializeToString()) == r
    payload = base64.b64encode(b"\x00\x01ckpt").decode()
    rep = P.TrainReply(message=payload)
    assert P.TrainReply.FromString(rep.SerializeToString()).message == payload


def test_descriptor_and_bytes_identical_to_reference(ref):
    theirs, ours = ref.rec, P.file_descriptor_proto()
    assert theirs["package"] == ours.package and theirs["syntax"] == ours.syntax
    assert [m["name"] for m in theirs["messages"]] == [m.name for m in ours.message_type]
    for mt, mo in zip(theirs["messages"], ours.message_type):
        assert [tuple(f) for f in mt["fields"]] == [(f.name, f.number, f.type, f.label) for f in mo.field]
    (so,) = ours.service
    assert theirs["service"]["name"] == so.name
    assert [tuple(m) for m in theirs["service"]["methods"]] == \
           [(m.name, m.input_type, m.output_type) for m in so.method]
    assert set(theirs["samples"]) == {name for name, _ in SAMPLES}
    for name, kw in SAMPLES:
        assert bytes.fromhex(theirs["samples"][name]) == getattr(P, name)(**kw).SerializeToString()
        assert getattr(ref, name)(**kw).SerializeToString() == bytes.fromhex(theirs["samples"][name])


class _Echo(P.TrainerServicer):
    def StartTrain(self, request, context):
        return P.TrainReply(message=f"{request.rank}/{request.world}")

    def HeartBeat(self, request, context):
        return P.HeartBeatResponse(status=1)


def test_reference_stub_talks_to_fedmi_server(ref):
    server = P.make_server(max_workers=2)
    P.add_TrainerServicer_to_server(_Echo(), server)
    port = server.add_insecure_port("127.0.0.1:0")
    server.start()
    try:
        ch = grpc.insecure_channel(f"127.0.0.1:{port}")
        stub = ref.stub(ch)
        assert stub.StartTrain(ref.TrainRequest(rank=1, world=4), timeout=5).message == "1/4"
        assert stub.HeartBeat(ref.Request(), timeout=5).status == 1
        with pytest.raises(grpc.RpcError) as ei:
            stub.SendModel(ref.SendModelRequest(model=""), timeout=5)
        assert ei.value.code() == grpc.StatusCode.UNIMPLEMENTED
    finally:
        server.stop(None)


def test_fedmi_stub_talks_to_reference_servicer(ref):
    class RefStyle:
        def CheckIfPrimaryUp(self, request, context):
            return ref.PingResponse(value=int(request.req) + 1)

    server = grpc.server(__import__("concurrent.futures").futures.ThreadPoolExecutor(2))
    ref.add_servicer_to_server(RefStyle(), server)
    port = server.add_insecure_port("127.0.0.1:0")
    server.start()
    try:
        stub = P.TrainerStub(P.make_channel(f"127.0.0.1:{port}", gzip=True))
        assert stub.CheckIfPrimaryUp(P.PingRequest(req="1"), timeout=5).value == 2
    finally:
        server.stop(None)
